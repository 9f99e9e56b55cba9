// libegs_sparsetsdf.so (include/egs_sparse_tsdf.h, which states every rule): the TSDF fusion and marching tetrahedra of
// libegs_tsdf.so on a block-allocated volume.  What a sample and a cell compute is egs_tsdf_device.h, shared
// with the dense kernels; here are the kernels around it:
//
//   k_touch            : a thread per pixel marches its ray through the truncation band and flags the blocks it meets
//                        (a same-value store of 1)
//   k_sparse_mark      : a thread per directory entry: unallocated and flagged within one block -> fresh
//   k_sparse_assign    : a thread per directory entry: a fresh block takes the slot the caller's scan gives it
//   k_sparse_integrate<COLOR, ALPHA, WEIGHT> : a thread owns a QUAD, four consecutive samples of a block's row (16 B of the
//                        pool, always aligned and whole); k_tsdf_integrate's body on it.  The (slot, quad) items are walked
//                        with the stride of the grid, which is capped.
//   k_sparse_count / k_sparse_emit : a workgroup per slot, a thread per cell; the block's 9^3 halo of tsdf and weight is
//                        staged in LDS (5.8 KB), the seven neighbours found through the directory
//
// No atomics: a sample and a cell's output are owned by one thread.
#define EGS_SIDE_LIBRARY "egs_sparsetsdf"
#include "egs_side_error.h"

#include <float.h>
#include <math.h>

#include "../../include/egs_sparse_tsdf.h"
#include "egs_tsdf_device.h"

namespace egs {

using egs_tsdf::Cell;
using egs_tsdf::Lattice;
using egs_tsdf::View;
using egs_tsdf::project_sample;

constexpr int ST_THREADS = 256;
constexpr int BLK = EGS_SPARSETSDF_BLOCK, BLK_N = EGS_SPARSETSDF_BLOCK_SAMPLES;
constexpr int HALO = BLK + 1, HALO_N = HALO * HALO * HALO;

struct Intrinsics { float fx, fy, cx, cy, trunc, alpha_min, near, depth_max; };
struct Blocks { int nbx, nby, nbz, n; };      // the block grid and its number of entries

template <bool ALPHA, bool WEIGHT>
__global__ __launch_bounds__(ST_THREADS) void k_touch(Lattice L, Blocks B, int H, int W, const float* __restrict__ depth,
                                                      const float* __restrict__ alpha,
                                                      const float* __restrict__ pixel_weight, Intrinsics K,
                                                      const float* __restrict__ Rcw, const float* __restrict__ tcw,
                                                      int32_t* __restrict__ flags) {
  const int64_t pix = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  if (pix >= (int64_t)H * W) return;
  const int py = (int)(pix / W), px = (int)(pix - (int64_t)py * W);
  // steps 3 and 5 of egs_tsdf.h, as decide_sample takes them
  float zs = depth[pix];
  if (ALPHA) {
    const float a = alpha[pix];
    if (!(a > K.alpha_min)) return;
    zs = zs / a;
  }
  if (!(zs > 0.f && zs <= FLT_MAX && zs <= K.depth_max)) return;
  if (WEIGHT) {
    const float w = pixel_weight[pix];
    if (!(w > 0.f && w <= FLT_MAX)) return;
  }
  const float z0 = fmaxf(K.near, zs - K.trunc), z1 = zs + K.trunc;
  const float nf = ceilf((z1 - z0) / L.voxel);
  if (!(nf >= 0.f)) return;
  const int n = nf < (float)(EGS_SPARSETSDF_MAX_MARCH + 1) ? (int)nf : EGS_SPARSETSDF_MAX_MARCH + 1;
  float R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rcw[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = tcw[k];
  const float dx = ((float)px - K.cx) / K.fx, dy = ((float)py - K.cy) / K.fy;
  const float o[3] = {L.ox, L.oy, L.oz};
  const int nb[3] = {B.nbx, B.nby, B.nbz};
  for (int k = 0; k <= n; ++k) {
    const float z = k < n ? fminf(z0 + (float)k * L.voxel, z1) : z1;
    const float pc[3] = {z * dx - t[0], z * dy - t[1], z - t[2]};
    int b[3];
    bool in = true;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const float pw = (R[ax] * pc[0] + R[3 + ax] * pc[1]) + R[6 + ax] * pc[2];      // R^T (p_c - t)
      const float i = floorf((pw - o[ax]) / L.voxel + 0.5f);
      // (false for NaN; the rim of one block around the grid is clamped onto it)
      in = in && i >= -(float)BLK && i < (float)(BLK * (nb[ax] + 1));
      const int bi = in ? ((int)i >> 3) : 0;
      b[ax] = bi < 0 ? 0 : bi > nb[ax] - 1 ? nb[ax] - 1 : bi;
    }
    if (in) flags[((int64_t)b[2] * B.nby + b[1]) * B.nbx + b[0]] = 1;
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_sparse_mark(Blocks B, const int32_t* __restrict__ flags,
                                                            const int32_t* __restrict__ directory,
                                                            int32_t* __restrict__ fresh) {
  const int b = blockIdx.x * ST_THREADS + threadIdx.x;
  if (b >= B.n) return;
  int hit = 0;
  if (directory[b] < 0) {
    const int bx = b % B.nbx, by = (b / B.nbx) % B.nby, bz = b / (B.nbx * B.nby);
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int x = bx + dx, y = by + dy, z = bz + dz;
          if (x >= 0 && x < B.nbx && y >= 0 && y < B.nby && z >= 0 && z < B.nbz)
            hit |= flags[(z * B.nby + y) * B.nbx + x] != 0 ? 1 : 0;
        }
  }
  fresh[b] = hit;
}

__global__ __launch_bounds__(ST_THREADS) void k_sparse_assign(Blocks B, const int32_t* __restrict__ fresh,
                                                              const int64_t* __restrict__ offsets, int n_blocks,
                                                              int capacity, int32_t* __restrict__ directory,
                                                              int32_t* __restrict__ block_coords) {
  const int b = blockIdx.x * ST_THREADS + threadIdx.x;
  if (b >= B.n || fresh[b] == 0) return;
  const int64_t off = offsets[b];
  if (off < 0 || off >= (int64_t)capacity - n_blocks) return;
  const int slot = n_blocks + (int)off;
  directory[b] = slot;
  block_coords[slot] = b;
}

template <bool COLOR, bool ALPHA, bool WEIGHT>
__global__ __launch_bounds__(ST_THREADS) void k_sparse_integrate(
    Lattice L, Blocks B, int n_blocks, int capacity, const int32_t* __restrict__ block_coords, float* __restrict__ tsdf,
    float* __restrict__ weight, float* __restrict__ color, int H, int W, const float* __restrict__ depth,
    const float* __restrict__ alpha, const float* __restrict__ image, const float* __restrict__ pixel_weight,
    Intrinsics K, const float* __restrict__ Rcw, const float* __restrict__ tcw) {
  View v;
  v.H = H; v.W = W;
  v.fx = K.fx; v.fy = K.fy; v.cx = K.cx; v.cy = K.cy;
  v.trunc = K.trunc; v.alpha_min = K.alpha_min; v.near = K.near; v.depth_max = K.depth_max;
#pragma unroll
  for (int k = 0; k < 9; ++k) v.R[k] = Rcw[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) v.t[k] = tcw[k];
  const int64_t plane = (int64_t)capacity * BLK_N, npix = (int64_t)H * W;
  // a block has 128 quads: items = 128 n_blocks <= 2^29
  const uint32_t n_items = (uint32_t)n_blocks * (BLK_N / 4), stride = gridDim.x * ST_THREADS;
  for (uint32_t item = blockIdx.x * ST_THREADS + threadIdx.x; item < n_items;) {
    const uint32_t slot = item >> 7, q = item & 127;
    item = item + stride < item ? n_items : item + stride;      // (the next one; a wrap ends the walk)
    const int32_t b = block_coords[slot];
    if ((uint32_t)b >= (uint32_t)B.n) continue;
    const int bx = b % B.nbx, by = (b / B.nbx) % B.nby, bz = b / (B.nbx * B.nby);
    const int xq = bx * BLK + (int)(q & 1) * 4, iy = by * BLK + (int)((q >> 1) & 7), iz = bz * BLK + (int)(q >> 4);
    if (xq >= L.nx || iy >= L.ny || iz >= L.nz) continue;
    const uint32_t lin = slot * BLK_N + q * 4;      // < 2^31
    // the four samples: project all, then all their gathers (a skipped sample reads pixel 0), then decide
    int pix[4];
    float pz[4], t[4], w[4], d[4], a[4], pw[4];
    bool upd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) upd[k] = project_sample(L, v, xq + k, iy, iz, pix[k], pz[k]) && xq + k < L.nx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k] = depth[pix[k]];
      a[k] = ALPHA ? alpha[pix[k]] : 1.f;
      pw[k] = WEIGHT ? pixel_weight[pix[k]] : 1.f;
    }
    bool any = false, all = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      t[k] = 0.f; w[k] = 0.f;
      upd[k] = upd[k] && egs_tsdf::decide_sample(v, pz[k], d[k], ALPHA, a[k], pw[k], t[k], w[k]);
      any = any || upd[k];
      all = all && upd[k];
    }
    if (!any) continue;
    const float4 f4 = *reinterpret_cast<const float4*>(tsdf + lin), w4 = *reinterpret_cast<const float4*>(weight + lin);
    const float f[4] = {f4.x, f4.y, f4.z, f4.w}, wt[4] = {w4.x, w4.y, w4.z, w4.w};
    float nf[4], nw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      nf[k] = egs_tsdf::blend(f[k], wt[k], t[k], w[k]);
      nw[k] = wt[k] + w[k];
    }
    if (all) {
      *reinterpret_cast<float4*>(tsdf + lin) = make_float4(nf[0], nf[1], nf[2], nf[3]);
      *reinterpret_cast<float4*>(weight + lin) = make_float4(nw[0], nw[1], nw[2], nw[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (upd[k]) {
          tsdf[lin + k] = nf[k];
          weight[lin + k] = nw[k];
        }
      }
    }
    if (COLOR) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* __restrict__ cp = color + c * plane + lin;
        const float* __restrict__ img = image + c * npix;
        const float4 c4 = *reinterpret_cast<const float4*>(cp);
        float col[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) col[k] = egs_tsdf::blend(col[k], wt[k], upd[k] ? img[pix[k]] : 0.f, w[k]);
        if (all) {
          *reinterpret_cast<float4*>(cp) = make_float4(col[0], col[1], col[2], col[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (upd[k]) cp[k] = col[k];
        }
      }
    }
  }
}

// where the corners of a cell of a block live (egs_tsdf_device.h): keys are those of the virtual lattice, the colours sit
// in the pool slot of the block the corner falls in, one of the eight in `nb` (LDS)
struct SparseAddr {
  int64_t sy, sz, plane;      // nx, nx ny; 512 capacity
  const int32_t* nb;
  int lx, ly, lz;
  __device__ __forceinline__ int64_t key(const Cell& c, int p) const {
    return c.base + (p & 1) + ((p >> 1) & 1) * sy + ((p >> 2) & 1) * sz;
  }
  __device__ __forceinline__ int64_t at(const Cell& c, int p) const {
    const int x = lx + (p & 1), y = ly + ((p >> 1) & 1), z = lz + ((p >> 2) & 1);
    const int slot = nb[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];      // (valid: the cell is meshed)
    return (int64_t)slot * BLK_N + ((z & 7) * 64 + (y & 7) * 8 + (x & 7));
  }
};

// Stage the halo of the workgroup's slot and load this thread's cell -> whether it is meshed.  Every thread of the
// workgroup calls it (barriers); `live` is false for a slot whose block index is out of range.
__device__ __forceinline__ bool load_block_cell(const Lattice& L, const Blocks& B, int n_blocks,
                                                const int32_t* __restrict__ directory,
                                                const int32_t* __restrict__ block_coords, const float* __restrict__ tsdf,
                                                const float* __restrict__ weight, float min_weight, int32_t* s_nb,
                                                float* s_f, float* s_w, Cell& c, SparseAddr& A) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  const int32_t b = block_coords[slot];
  const bool live = (uint32_t)b < (uint32_t)B.n;
  const int bx = live ? b % B.nbx : 0, by = live ? (b / B.nbx) % B.nby : 0, bz = live ? b / (B.nbx * B.nby) : 0;
  if (tid < 8) {
    const int x = bx + (tid & 1), y = by + ((tid >> 1) & 1), z = bz + ((tid >> 2) & 1);
    int s = -1;
    if (live && x < B.nbx && y < B.nby && z < B.nbz) s = tid == 0 ? slot : directory[(z * B.nby + y) * B.nbx + x];
    s_nb[tid] = s >= 0 && s < n_blocks ? s : -1;
  }
  __syncthreads();
  for (int h = tid; h < HALO_N; h += BLK_N) {
    const int hx = h % HALO, hy = (h / HALO) % HALO, hz = h / (HALO * HALO);
    const int s = s_nb[(hx >> 3) | ((hy >> 3) << 1) | ((hz >> 3) << 2)];
    const bool ok = s >= 0 && bx * BLK + hx < L.nx && by * BLK + hy < L.ny && bz * BLK + hz < L.nz;
    const uint32_t at = (uint32_t)(ok ? s : 0) * BLK_N + ((hz & 7) * 64 + (hy & 7) * 8 + (hx & 7));
    // (a corner outside the lattice or in an unallocated block: weight 0 is below every min_weight)
    s_f[h] = ok ? tsdf[at] : 1.f;
    s_w[h] = ok ? weight[at] : 0.f;
  }
  __syncthreads();
  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  c.cx = bx * BLK + lx; c.cy = by * BLK + ly; c.cz = bz * BLK + lz;
  c.base = ((int64_t)c.cz * L.ny + c.cy) * L.nx + c.cx;
  bool valid = live;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int h = ((lz + ((k >> 2) & 1)) * HALO + (ly + ((k >> 1) & 1))) * HALO + (lx + (k & 1));
    valid = valid && s_w[h] >= min_weight;
    c.f[k] = s_f[h];
  }
  A.sy = L.nx; A.sz = (int64_t)L.nx * L.ny;
  A.nb = s_nb;
  A.lx = lx; A.ly = ly; A.lz = lz;
  return valid;
}

__global__ __launch_bounds__(BLK_N) void k_sparse_count(Lattice L, Blocks B, int n_blocks,
                                                        const int32_t* __restrict__ directory,
                                                        const int32_t* __restrict__ block_coords,
                                                        const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                        float min_weight, int32_t* __restrict__ counts) {
  __shared__ int32_t s_nb[8];
  __shared__ float s_f[HALO_N], s_w[HALO_N];
  Cell c;
  SparseAddr A;
  int n = 0;
  if (load_block_cell(L, B, n_blocks, directory, block_coords, tsdf, weight, min_weight, s_nb, s_f, s_w, c, A)) {
    int inside8 = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) inside8 |= (c.f[k] < 0.f ? 1 : 0) << k;
    n = egs_tsdf::cell_triangles(inside8);
  }
  counts[(int64_t)blockIdx.x * BLK_N + threadIdx.x] = n;
}

// where a cell's triangles go: triangle k of the cell is triangle first + k of the mesh, and none at or past `total`
struct MeshOut {
  float* __restrict__ verts;
  int64_t* __restrict__ keys;
  float* __restrict__ colors;
  int64_t first, total, tri;
  __device__ __forceinline__ bool begin(int k) {
    tri = first + k;
    return tri >= 0 && tri < total;
  }
  __device__ __forceinline__ void vertex(int slot, float x, float y, float z, int64_t key) {
    float* p = verts + (tri * 3 + slot) * 3;
    p[0] = x; p[1] = y; p[2] = z;
    keys[tri * 3 + slot] = key;
  }
  __device__ __forceinline__ void colour(int slot, float r, float g, float b) {
    float* p = colors + (tri * 3 + slot) * 3;
    p[0] = r; p[1] = g; p[2] = b;
  }
};

__global__ __launch_bounds__(BLK_N) void k_sparse_emit(Lattice L, Blocks B, int n_blocks, int capacity,
                                                       const int32_t* __restrict__ directory,
                                                       const int32_t* __restrict__ block_coords,
                                                       const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                       const float* __restrict__ color, float min_weight,
                                                       const int64_t* __restrict__ offsets, int64_t total,
                                                       float* __restrict__ verts, int64_t* __restrict__ keys,
                                                       float* __restrict__ colors) {
  __shared__ int32_t s_nb[8];
  __shared__ float s_f[HALO_N], s_w[HALO_N];
  Cell c;
  SparseAddr A;
  if (!load_block_cell(L, B, n_blocks, directory, block_coords, tsdf, weight, min_weight, s_nb, s_f, s_w, c, A)) return;
  A.plane = (int64_t)capacity * BLK_N;
  MeshOut out = {verts, keys, colors, offsets[(int64_t)blockIdx.x * BLK_N + threadIdx.x], total, 0};
  egs_tsdf::emit_cell(L, c, color, A, out);
}

}  // namespace egs

using namespace egs;

static bool aligned_to(const void* a, uintptr_t k) { return ((uintptr_t)a & (k - 1)) == 0; }
static bool finite_f(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }
static bool positive_f(float v) { return v > 0.f && v <= FLT_MAX; }
static int64_t blocks_of(int n) { return ((int64_t)n + EGS_SPARSETSDF_BLOCK - 1) / EGS_SPARSETSDF_BLOCK; }
static bool lattice_ok(int nx, int ny, int nz) {
  return nx > 0 && ny > 0 && nz > 0 && blocks_of(nx) * blocks_of(ny) <= EGS_SPARSETSDF_MAX_DIRECTORY &&
         blocks_of(nx) * blocks_of(ny) * blocks_of(nz) <= EGS_SPARSETSDF_MAX_DIRECTORY;
}
static Blocks blocks(int nx, int ny, int nz) {
  const Blocks B = {(int)blocks_of(nx), (int)blocks_of(ny), (int)blocks_of(nz),
                    (int)(blocks_of(nx) * blocks_of(ny) * blocks_of(nz))};
  return B;
}
static bool pool_ok(int n_blocks, int capacity) {
  return n_blocks >= 0 && n_blocks <= capacity && capacity <= EGS_SPARSETSDF_MAX_SLOTS;
}

extern "C" int egs_sparsetsdf_abi_version(void) { return EGS_SPARSETSDF_ABI_VERSION; }
extern "C" const char* egs_sparsetsdf_last_error_string(void) { return egs_side::g_err; }

#define SIDE_CHECK_VIEW()                                                                         \
  SIDE_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31));                          \
  SIDE_CHECK_ARG(depth != nullptr && aligned_to(depth, 4));                                       \
  SIDE_CHECK_ARG(aligned_to(alpha, 4) && aligned_to(pixel_weight, 4));                            \
  SIDE_CHECK_ARG(positive_f(fx) && positive_f(fy) && finite_f(cx) && finite_f(cy));               \
  SIDE_CHECK_ARG(Rcw != nullptr && aligned_to(Rcw, 4) && tcw != nullptr && aligned_to(tcw, 4));   \
  SIDE_CHECK_ARG(positive_f(trunc));                                                              \
  SIDE_CHECK_ARG(alpha_min >= 0.f && alpha_min <= FLT_MAX && near >= 0.f && near <= FLT_MAX);     \
  SIDE_CHECK_ARG(depth_max > 0.f) /* (+inf: no limit; false for NaN) */

extern "C" int egs_sparsetsdf_touch(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int H, int W,
                                    const float* depth, const float* alpha, const float* pixel_weight, float fx, float fy,
                                    float cx, float cy, const float* Rcw, const float* tcw, float trunc, float alpha_min,
                                    float near, float depth_max, int32_t* flags, void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(finite_f(ox) && finite_f(oy) && finite_f(oz) && positive_f(voxel));
  SIDE_CHECK_VIEW();
  SIDE_CHECK_ARG(2.f * trunc <= (float)EGS_SPARSETSDF_MAX_MARCH * voxel);
  SIDE_CHECK_ARG(flags != nullptr && aligned_to(flags, 4));
  for (const void* in : {(const void*)depth, (const void*)alpha, (const void*)pixel_weight, (const void*)Rcw,
                         (const void*)tcw})
    SIDE_CHECK_ARG((const void*)flags != in);
  const Lattice L = {nx, ny, nz, ox, oy, oz, voxel};
  const Intrinsics K = {fx, fy, cx, cy, trunc, alpha_min, near, depth_max};
  const Blocks B = blocks(nx, ny, nz);
  const int grid = (int)(((int64_t)H * W + ST_THREADS - 1) / ST_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (alpha && pixel_weight)
    hipLaunchKernelGGL((k_touch<true, true>), dim3(grid), dim3(ST_THREADS), 0, s, L, B, H, W, depth, alpha, pixel_weight,
                       K, Rcw, tcw, flags);
  else if (alpha)
    hipLaunchKernelGGL((k_touch<true, false>), dim3(grid), dim3(ST_THREADS), 0, s, L, B, H, W, depth, alpha, pixel_weight,
                       K, Rcw, tcw, flags);
  else if (pixel_weight)
    hipLaunchKernelGGL((k_touch<false, true>), dim3(grid), dim3(ST_THREADS), 0, s, L, B, H, W, depth, alpha, pixel_weight,
                       K, Rcw, tcw, flags);
  else
    hipLaunchKernelGGL((k_touch<false, false>), dim3(grid), dim3(ST_THREADS), 0, s, L, B, H, W, depth, alpha,
                       pixel_weight, K, Rcw, tcw, flags);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_sparsetsdf_mark(int nx, int ny, int nz, const int32_t* flags, const int32_t* directory, int32_t* fresh,
                                   void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(flags != nullptr && aligned_to(flags, 4) && directory != nullptr && aligned_to(directory, 4));
  SIDE_CHECK_ARG(fresh != nullptr && aligned_to(fresh, 4) && fresh != flags && fresh != directory);
  const Blocks B = blocks(nx, ny, nz);
  hipLaunchKernelGGL(k_sparse_mark, dim3((B.n + ST_THREADS - 1) / ST_THREADS), dim3(ST_THREADS), 0, (hipStream_t)stream,
                     B, flags, directory, fresh);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_sparsetsdf_assign(int nx, int ny, int nz, const int32_t* fresh, const int64_t* offsets, int n_blocks,
                                     int capacity, int32_t* directory, int32_t* block_coords, void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(pool_ok(n_blocks, capacity));
  SIDE_CHECK_ARG(fresh != nullptr && aligned_to(fresh, 4) && offsets != nullptr && aligned_to(offsets, 8));
  SIDE_CHECK_ARG(directory != nullptr && aligned_to(directory, 4) && directory != fresh &&
                 (const void*)directory != (const void*)offsets);
  if (capacity == n_blocks) return 0;      // no room for a new slot: nothing to write
  SIDE_CHECK_ARG(block_coords != nullptr && aligned_to(block_coords, 4) && block_coords != fresh &&
                 (const void*)block_coords != (const void*)offsets && block_coords != directory);
  const Blocks B = blocks(nx, ny, nz);
  hipLaunchKernelGGL(k_sparse_assign, dim3((B.n + ST_THREADS - 1) / ST_THREADS), dim3(ST_THREADS), 0,
                     (hipStream_t)stream, B, fresh, offsets, n_blocks, capacity, directory, block_coords);
  SIDE_HIP(hipGetLastError());
  return 0;
}

template <bool COLOR, bool ALPHA>
static void launch_integrate(bool weighted, int grid, hipStream_t s, const Lattice& L, const Blocks& B, int n_blocks,
                             int capacity, const int32_t* block_coords, float* tsdf, float* weight, float* color, int H,
                             int W, const float* depth, const float* alpha, const float* image, const float* pw,
                             const Intrinsics& K, const float* Rcw, const float* tcw) {
  if (weighted)
    hipLaunchKernelGGL((k_sparse_integrate<COLOR, ALPHA, true>), dim3(grid), dim3(ST_THREADS), 0, s, L, B, n_blocks,
                       capacity, block_coords, tsdf, weight, color, H, W, depth, alpha, image, pw, K, Rcw, tcw);
  else
    hipLaunchKernelGGL((k_sparse_integrate<COLOR, ALPHA, false>), dim3(grid), dim3(ST_THREADS), 0, s, L, B, n_blocks,
                       capacity, block_coords, tsdf, weight, color, H, W, depth, alpha, image, pw, K, Rcw, tcw);
}

extern "C" int egs_sparsetsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int n_blocks,
                                        int capacity, const int32_t* block_coords, float* tsdf, float* weight,
                                        float* color, int H, int W, const float* depth, const float* alpha,
                                        const float* image, const float* pixel_weight, float fx, float fy, float cx,
                                        float cy, const float* Rcw, const float* tcw, float trunc, float alpha_min,
                                        float near, float depth_max, int max_blocks, void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(finite_f(ox) && finite_f(oy) && finite_f(oz) && positive_f(voxel));
  SIDE_CHECK_ARG(pool_ok(n_blocks, capacity));
  SIDE_CHECK_ARG(aligned_to(block_coords, 4));
  SIDE_CHECK_ARG(tsdf != nullptr && aligned_to(tsdf, 16));
  SIDE_CHECK_ARG(weight != nullptr && aligned_to(weight, 16) && weight != tsdf);
  SIDE_CHECK_ARG(aligned_to(color, 16) && (color == nullptr || (color != tsdf && color != weight)));
  SIDE_CHECK_VIEW();
  SIDE_CHECK_ARG(aligned_to(image, 4));
  SIDE_CHECK_ARG((color == nullptr) == (image == nullptr));
  SIDE_CHECK_ARG(max_blocks >= 0 && max_blocks <= EGS_SPARSETSDF_MAX_BLOCKS);
  for (const float* out : {(const float*)tsdf, (const float*)weight, (const float*)color})
    if (out)
      SIDE_CHECK_ARG(out != depth && out != alpha && out != image && out != pixel_weight && out != Rcw && out != tcw &&
                     (const void*)out != (const void*)block_coords);
  if (n_blocks == 0) return 0;
  SIDE_CHECK_ARG(block_coords != nullptr);
  const Lattice L = {nx, ny, nz, ox, oy, oz, voxel};
  const Intrinsics K = {fx, fy, cx, cy, trunc, alpha_min, near, depth_max};
  const Blocks B = blocks(nx, ny, nz);
  const int64_t items = (int64_t)n_blocks * (EGS_SPARSETSDF_BLOCK_SAMPLES / 4);
  const int cap = max_blocks > 0 ? max_blocks : EGS_SPARSETSDF_MAX_BLOCKS;
  const int64_t want = (items + ST_THREADS - 1) / ST_THREADS;
  const int grid = (int)(want < cap ? want : cap);
  hipStream_t s = (hipStream_t)stream;
  const bool weighted = pixel_weight != nullptr;
  if (color && alpha)
    launch_integrate<true, true>(weighted, grid, s, L, B, n_blocks, capacity, block_coords, tsdf, weight, color, H, W,
                                 depth, alpha, image, pixel_weight, K, Rcw, tcw);
  else if (color)
    launch_integrate<true, false>(weighted, grid, s, L, B, n_blocks, capacity, block_coords, tsdf, weight, color, H, W,
                                  depth, alpha, image, pixel_weight, K, Rcw, tcw);
  else if (alpha)
    launch_integrate<false, true>(weighted, grid, s, L, B, n_blocks, capacity, block_coords, tsdf, weight, color, H, W,
                                  depth, alpha, image, pixel_weight, K, Rcw, tcw);
  else
    launch_integrate<false, false>(weighted, grid, s, L, B, n_blocks, capacity, block_coords, tsdf, weight, color, H, W,
                                   depth, alpha, image, pixel_weight, K, Rcw, tcw);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_sparsetsdf_mesh_count(int nx, int ny, int nz, int n_blocks, int capacity, const int32_t* directory,
                                         const int32_t* block_coords, const float* tsdf, const float* weight,
                                         float min_weight, int32_t* counts, void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(pool_ok(n_blocks, capacity));
  SIDE_CHECK_ARG(directory != nullptr && aligned_to(directory, 4) && aligned_to(block_coords, 4));
  SIDE_CHECK_ARG(tsdf != nullptr && aligned_to(tsdf, 4) && weight != nullptr && aligned_to(weight, 4));
  SIDE_CHECK_ARG(positive_f(min_weight));
  if (n_blocks == 0) return 0;
  SIDE_CHECK_ARG(block_coords != nullptr && counts != nullptr && aligned_to(counts, 4));
  for (const void* in : {(const void*)directory, (const void*)block_coords, (const void*)tsdf, (const void*)weight})
    SIDE_CHECK_ARG((const void*)counts != in);
  const Lattice L = {nx, ny, nz, 0.f, 0.f, 0.f, 1.f};
  hipLaunchKernelGGL(k_sparse_count, dim3(n_blocks), dim3(EGS_SPARSETSDF_BLOCK_SAMPLES), 0, (hipStream_t)stream, L,
                     blocks(nx, ny, nz), n_blocks, directory, block_coords, tsdf, weight, min_weight, counts);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_sparsetsdf_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int n_blocks,
                                        int capacity, const int32_t* directory, const int32_t* block_coords,
                                        const float* tsdf, const float* weight, const float* color, float min_weight,
                                        const int64_t* offsets, int64_t total, int64_t out_capacity, float* verts,
                                        int64_t* keys, float* colors, void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(finite_f(ox) && finite_f(oy) && finite_f(oz) && positive_f(voxel));
  SIDE_CHECK_ARG(pool_ok(n_blocks, capacity));
  SIDE_CHECK_ARG(directory != nullptr && aligned_to(directory, 4) && aligned_to(block_coords, 4));
  SIDE_CHECK_ARG(tsdf != nullptr && aligned_to(tsdf, 4) && weight != nullptr && aligned_to(weight, 4));
  SIDE_CHECK_ARG(aligned_to(color, 4) && (color == nullptr) == (colors == nullptr));
  SIDE_CHECK_ARG(positive_f(min_weight));
  SIDE_CHECK_ARG(total >= 0 && total < ((int64_t)1 << 31) && out_capacity >= 0);
  SIDE_CHECK_ARG(total <= (int64_t)n_blocks * EGS_SPARSETSDF_BLOCK_SAMPLES * 12);
  if (out_capacity < total) {
    egs_side::set_error(EGS_SPARSETSDF_ERR_CAPACITY, "the mesh buffers hold fewer triangles than the scan's total",
                        __FILE__, __LINE__);
    return EGS_SPARSETSDF_ERR_CAPACITY;
  }
  if (total == 0) return 0;
  SIDE_CHECK_ARG(block_coords != nullptr && offsets != nullptr && aligned_to(offsets, 8));
  SIDE_CHECK_ARG(verts != nullptr && aligned_to(verts, 4) && keys != nullptr && aligned_to(keys, 8));
  SIDE_CHECK_ARG(aligned_to(colors, 4) && (const void*)verts != (const void*)keys && colors != verts &&
                 (const void*)colors != (const void*)keys);
  for (const void* out : {(const void*)verts, (const void*)keys, (const void*)colors})
    if (out)
      SIDE_CHECK_ARG(out != tsdf && out != weight && out != color && out != offsets && out != directory &&
                     out != block_coords);
  const Lattice L = {nx, ny, nz, ox, oy, oz, voxel};
  hipLaunchKernelGGL(k_sparse_emit, dim3(n_blocks), dim3(EGS_SPARSETSDF_BLOCK_SAMPLES), 0, (hipStream_t)stream, L,
                     blocks(nx, ny, nz), n_blocks, capacity, directory, block_coords, tsdf, weight, color, min_weight,
                     offsets, total, verts, keys, colors);
  SIDE_HIP(hipGetLastError());
  return 0;
}
