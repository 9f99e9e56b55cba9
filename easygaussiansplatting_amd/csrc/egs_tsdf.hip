// libegs_tsdf.so (include/egs_tsdf.h, which states every rule): fusion of depth maps into a truncated signed distance
// volume and extraction of its zero level set by marching tetrahedra.  What a sample and a cell compute is
// in egs_tsdf_device.h; here are the three kernels around it:
//
//   k_tsdf_integrate<COLOR, ALPHA, WEIGHT> : a thread owns four consecutive samples of one (iy, iz) row of the sub-box: a
//                    QUAD, aligned to 16 B in the plane (so a row with nx % 4 != 0 starts and ends with ragged quads).
//                    It decides its four samples first -- projection and the gathers from the maps, no plane traffic --
//                    and touches the planes only if one of them is updated: one 16-B load per plane, and one 16-B store
//                    when all four are updated, scalar stores of the updated ones otherwise (a skipped sample is never
//                    written).  The (row, quad) items are walked with the stride of the grid, which is capped.
//   k_mesh_count   : a thread per cell: its number of triangles
//   k_mesh_emit    : a thread per cell: its triangles at the offset the caller's exclusive scan gives it
//
// No atomics, no LDS: a sample and a cell's output are owned by one thread.
#define EGS_SIDE_LIBRARY "egs_tsdf"
#include "egs_side_error.h"

#include <float.h>
#include <math.h>

#include "../../include/egs_tsdf.h"
#include "egs_tsdf_device.h"

namespace egs {

using egs_tsdf::Cell;
using egs_tsdf::Lattice;
using egs_tsdf::View;
using egs_tsdf::project_sample;

constexpr int TSDF_THREADS = 256;

struct Box { int x0, x1, y0, y1, z0, z1; };
struct Intrinsics { float fx, fy, cx, cy, trunc, alpha_min, near, depth_max; };

template <bool COLOR, bool ALPHA, bool WEIGHT>
__global__ __launch_bounds__(TSDF_THREADS) void k_tsdf_integrate(
    Lattice L, Box box, int quads_per_row, int64_t items, float* __restrict__ tsdf, float* __restrict__ weight,
    float* __restrict__ color, int H, int W, const float* __restrict__ depth, const float* __restrict__ alpha,
    const float* __restrict__ image, const float* __restrict__ pixel_weight, Intrinsics K,
    const float* __restrict__ Rcw, const float* __restrict__ tcw) {
  View v;
  v.H = H; v.W = W;
  v.fx = K.fx; v.fy = K.fy; v.cx = K.cx; v.cy = K.cy;
  v.trunc = K.trunc; v.alpha_min = K.alpha_min; v.near = K.near; v.depth_max = K.depth_max;
#pragma unroll
  for (int k = 0; k < 9; ++k) v.R[k] = Rcw[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) v.t[k] = tcw[k];
  const int64_t total = (int64_t)L.nx * L.ny * L.nz, npix = (int64_t)H * W;
  const bool planes_aligned = (total & 3) == 0;      // colour plane c starts at c * total floats
  // (items < 2^32: a row has at most nx / 4 + 2 quads and nx ny nz < 2^31 -- 32-bit index arithmetic, no 64-bit division)
  const uint32_t rows_y = (uint32_t)(box.y1 - box.y0), qpr = (uint32_t)quads_per_row, n_items = (uint32_t)items;
  const uint32_t stride = gridDim.x * TSDF_THREADS;
  for (uint32_t item = blockIdx.x * TSDF_THREADS + threadIdx.x; item < n_items;) {
    const uint32_t row = item / qpr, q = item - row * qpr, rz = row / rows_y;
    const int iy = box.y0 + (int)(row - rz * rows_y), iz = box.z0 + (int)rz;
    item = item + stride < item ? n_items : item + stride;      // (the next one; a wrap ends the walk)
    const int64_t row_base = ((int64_t)iz * L.ny + iy) * L.nx;
    // the q-th aligned quad that meets [row_base + x0, row_base + x1)
    const int64_t first = (row_base + box.x0) & ~(int64_t)3;
    const int64_t lin = first + 4 * (int64_t)q;
    const int xq = (int)(lin - row_base);      // x of the quad's sample 0: may be < x0, or < 0
    if (xq >= box.x1) continue;
    // the four samples: project all, then all their gathers (a skipped sample reads pixel 0), then decide
    int pix[4];
    float pz[4], t[4], w[4], d[4], a[4], pw[4];
    bool upd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ix = xq + k;
      upd[k] = project_sample(L, v, ix, iy, iz, pix[k], pz[k]) && ix >= box.x0 && ix < box.x1;
    }
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
    // (a quad lies inside the plane except the last one of a volume with total % 4 != 0: reading the samples of a
    // neighbouring row is harmless, only the updated ones are written)
    const bool whole = lin + 4 <= total;
    float f[4], wt[4];
    if (whole) {
      const float4 a = *reinterpret_cast<const float4*>(tsdf + lin), b = *reinterpret_cast<const float4*>(weight + lin);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
      wt[0] = b.x; wt[1] = b.y; wt[2] = b.z; wt[3] = b.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        f[k] = upd[k] ? tsdf[lin + k] : 0.f;
        wt[k] = upd[k] ? weight[lin + k] : 0.f;
      }
    }
    float nf[4], nw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      nf[k] = egs_tsdf::blend(f[k], wt[k], t[k], w[k]);
      nw[k] = wt[k] + w[k];
    }
    if (all && whole) {
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
        float* __restrict__ plane = color + c * total;
        const float* __restrict__ img = image + c * npix;
        float col[4];
        if (whole && planes_aligned) {
          const float4 a = *reinterpret_cast<const float4*>(plane + lin);
          col[0] = a.x; col[1] = a.y; col[2] = a.z; col[3] = a.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) col[k] = upd[k] ? plane[lin + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) col[k] = egs_tsdf::blend(col[k], wt[k], upd[k] ? img[pix[k]] : 0.f, w[k]);
        if (all && whole && planes_aligned) {
          *reinterpret_cast<float4*>(plane + lin) = make_float4(col[0], col[1], col[2], col[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (upd[k]) plane[lin + k] = col[k];
        }
      }
    }
  }
}

// the corners of cell `cell`: -> false if one of them has weight < min_weight (or a NaN weight)
__device__ __forceinline__ bool load_cell(int nx, int ny, int nz, int64_t cell, const float* __restrict__ tsdf,
                                          const float* __restrict__ weight, float min_weight, Cell& c) {
  const int cnx = nx - 1, cny = ny - 1;
  c.cx = (int)(cell % cnx);
  c.cy = (int)((cell / cnx) % cny);
  c.cz = (int)(cell / ((int64_t)cnx * cny));
  c.base = ((int64_t)c.cz * ny + c.cy) * nx + c.cx;
  bool valid = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t i = c.base + (k & 1) + (int64_t)((k >> 1) & 1) * nx + (int64_t)((k >> 2) & 1) * nx * ny;
    valid = valid && weight[i] >= min_weight;
    c.f[k] = tsdf[i];
  }
  return valid;
}

__global__ __launch_bounds__(TSDF_THREADS) void k_mesh_count(int nx, int ny, int nz, int64_t cells,
                                                             const float* __restrict__ tsdf,
                                                             const float* __restrict__ weight, float min_weight,
                                                             int32_t* __restrict__ counts) {
  const int64_t cell = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (cell >= cells) return;
  Cell c;
  int n = 0;
  if (load_cell(nx, ny, nz, cell, tsdf, weight, min_weight, c)) {
    int inside8 = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) inside8 |= (c.f[k] < 0.f ? 1 : 0) << k;
    n = egs_tsdf::cell_triangles(inside8);
  }
  counts[cell] = n;
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

__global__ __launch_bounds__(TSDF_THREADS) void k_mesh_emit(Lattice L, int64_t cells, const float* __restrict__ tsdf,
                                                            const float* __restrict__ weight,
                                                            const float* __restrict__ color, float min_weight,
                                                            const int64_t* __restrict__ offsets, int64_t total,
                                                            float* __restrict__ verts, int64_t* __restrict__ keys,
                                                            float* __restrict__ colors) {
  const int64_t cell = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (cell >= cells) return;
  Cell c;
  if (!load_cell(L.nx, L.ny, L.nz, cell, tsdf, weight, min_weight, c)) return;
  MeshOut out = {verts, keys, colors, offsets[cell], total, 0};
  const egs_tsdf::DenseAddr addr = {L.nx, (int64_t)L.nx * L.ny, (int64_t)L.nx * L.ny * L.nz};
  egs_tsdf::emit_cell(L, c, color, addr, out);
}

}  // namespace egs

using namespace egs;

static bool aligned_to(const void* a, uintptr_t k) { return ((uintptr_t)a & (k - 1)) == 0; }
static bool finite_f(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }
static bool positive_f(float v) { return v > 0.f && v <= FLT_MAX; }
static bool lattice_ok(int nx, int ny, int nz) {
  return nx > 0 && ny > 0 && nz > 0 && (int64_t)nx * ny < ((int64_t)1 << 31) &&
         (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}
static int64_t cells_of(int nx, int ny, int nz) { return (int64_t)(nx - 1) * (ny - 1) * (nz - 1); }

extern "C" int egs_tsdf_abi_version(void) { return EGS_TSDF_ABI_VERSION; }
extern "C" const char* egs_tsdf_last_error_string(void) { return egs_side::g_err; }

template <bool COLOR, bool ALPHA>
static void launch_integrate(bool weighted, int grid, hipStream_t s, const Lattice& L, const Box& box, int qpr,
                             int64_t items, float* tsdf, float* weight, float* color, int H, int W, const float* depth,
                             const float* alpha, const float* image, const float* pw, const Intrinsics& K,
                             const float* Rcw, const float* tcw) {
  if (weighted)
    hipLaunchKernelGGL((k_tsdf_integrate<COLOR, ALPHA, true>), dim3(grid), dim3(TSDF_THREADS), 0, s, L, box, qpr, items,
                       tsdf, weight, color, H, W, depth, alpha, image, pw, K, Rcw, tcw);
  else
    hipLaunchKernelGGL((k_tsdf_integrate<COLOR, ALPHA, false>), dim3(grid), dim3(TSDF_THREADS), 0, s, L, box, qpr, items,
                       tsdf, weight, color, H, W, depth, alpha, image, pw, K, Rcw, tcw);
}

extern "C" int egs_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int x0, int x1,
                                  int y0, int y1, int z0, int z1, float* tsdf, float* weight, float* color, int H, int W,
                                  const float* depth, const float* alpha, const float* image, const float* pixel_weight,
                                  float fx, float fy, float cx, float cy, const float* Rcw, const float* tcw, float trunc,
                                  float alpha_min, float near, float depth_max, int max_blocks, void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(finite_f(ox) && finite_f(oy) && finite_f(oz) && positive_f(voxel));
  SIDE_CHECK_ARG(0 <= x0 && x0 <= x1 && x1 <= nx);
  SIDE_CHECK_ARG(0 <= y0 && y0 <= y1 && y1 <= ny);
  SIDE_CHECK_ARG(0 <= z0 && z0 <= z1 && z1 <= nz);
  SIDE_CHECK_ARG(tsdf != nullptr && aligned_to(tsdf, 16));
  SIDE_CHECK_ARG(weight != nullptr && aligned_to(weight, 16) && weight != tsdf);
  SIDE_CHECK_ARG(aligned_to(color, 16) && (color == nullptr || (color != tsdf && color != weight)));
  SIDE_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31));
  SIDE_CHECK_ARG(depth != nullptr && aligned_to(depth, 4));
  SIDE_CHECK_ARG(aligned_to(alpha, 4) && aligned_to(image, 4) && aligned_to(pixel_weight, 4));
  SIDE_CHECK_ARG((color == nullptr) == (image == nullptr));
  SIDE_CHECK_ARG(positive_f(fx) && positive_f(fy) && finite_f(cx) && finite_f(cy));
  SIDE_CHECK_ARG(Rcw != nullptr && aligned_to(Rcw, 4) && tcw != nullptr && aligned_to(tcw, 4));
  SIDE_CHECK_ARG(positive_f(trunc));
  SIDE_CHECK_ARG(alpha_min >= 0.f && alpha_min <= FLT_MAX && near >= 0.f && near <= FLT_MAX);
  SIDE_CHECK_ARG(depth_max > 0.f);      // (+inf: no limit; false for NaN)
  SIDE_CHECK_ARG(max_blocks >= 0 && max_blocks <= EGS_TSDF_MAX_BLOCKS);
  for (const float* out : {(const float*)tsdf, (const float*)weight, (const float*)color})
    if (out)
      SIDE_CHECK_ARG(out != depth && out != alpha && out != image && out != pixel_weight && out != Rcw && out != tcw);
  if (x0 == x1 || y0 == y1 || z0 == z1) return 0;
  const Lattice L = {nx, ny, nz, ox, oy, oz, voxel};
  const Box box = {x0, x1, y0, y1, z0, z1};
  const Intrinsics K = {fx, fy, cx, cy, trunc, alpha_min, near, depth_max};
  // aligned quads that can meet a row's [x0, x1): the row's first quad starts up to three samples before x0
  const int qpr = (x1 - x0 + 3) / 4 + 1;
  const int64_t items = (int64_t)(y1 - y0) * (z1 - z0) * qpr;
  const int cap = max_blocks > 0 ? max_blocks : EGS_TSDF_MAX_BLOCKS;
  const int64_t want = (items + TSDF_THREADS - 1) / TSDF_THREADS;
  const int grid = (int)(want < cap ? want : cap);
  hipStream_t s = (hipStream_t)stream;
  const bool weighted = pixel_weight != nullptr;
  if (color && alpha)
    launch_integrate<true, true>(weighted, grid, s, L, box, qpr, items, tsdf, weight, color, H, W, depth, alpha, image,
                                 pixel_weight, K, Rcw, tcw);
  else if (color)
    launch_integrate<true, false>(weighted, grid, s, L, box, qpr, items, tsdf, weight, color, H, W, depth, alpha, image,
                                  pixel_weight, K, Rcw, tcw);
  else if (alpha)
    launch_integrate<false, true>(weighted, grid, s, L, box, qpr, items, tsdf, weight, color, H, W, depth, alpha, image,
                                  pixel_weight, K, Rcw, tcw);
  else
    launch_integrate<false, false>(weighted, grid, s, L, box, qpr, items, tsdf, weight, color, H, W, depth, alpha, image,
                                   pixel_weight, K, Rcw, tcw);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_tsdf_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float min_weight,
                                   int32_t* counts, void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(tsdf != nullptr && aligned_to(tsdf, 4) && weight != nullptr && aligned_to(weight, 4));
  SIDE_CHECK_ARG(positive_f(min_weight));
  const int64_t cells = cells_of(nx, ny, nz);
  if (cells == 0) return 0;
  SIDE_CHECK_ARG(counts != nullptr && aligned_to(counts, 4));
  SIDE_CHECK_ARG((const void*)counts != (const void*)tsdf && (const void*)counts != (const void*)weight);
  const int grid = (int)((cells + TSDF_THREADS - 1) / TSDF_THREADS);
  hipLaunchKernelGGL(k_mesh_count, dim3(grid), dim3(TSDF_THREADS), 0, (hipStream_t)stream, nx, ny, nz, cells, tsdf,
                     weight, min_weight, counts);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_tsdf_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* tsdf,
                                  const float* weight, const float* color, float min_weight, const int64_t* offsets,
                                  int64_t total, int64_t capacity, float* verts, int64_t* keys, float* colors,
                                  void* stream) {
  SIDE_CHECK_ARG(lattice_ok(nx, ny, nz));
  SIDE_CHECK_ARG(finite_f(ox) && finite_f(oy) && finite_f(oz) && positive_f(voxel));
  SIDE_CHECK_ARG(tsdf != nullptr && aligned_to(tsdf, 4) && weight != nullptr && aligned_to(weight, 4));
  SIDE_CHECK_ARG(aligned_to(color, 4) && (color == nullptr) == (colors == nullptr));
  SIDE_CHECK_ARG(positive_f(min_weight));
  SIDE_CHECK_ARG(total >= 0 && total < ((int64_t)1 << 31) && capacity >= 0);
  const int64_t cells = cells_of(nx, ny, nz);
  SIDE_CHECK_ARG(total <= cells * EGS_TSDF_CELL_TRIANGLES);
  if (capacity < total) {
    egs_side::set_error(EGS_TSDF_ERR_CAPACITY, "the mesh buffers hold fewer triangles than the scan's total", __FILE__,
                        __LINE__);
    return EGS_TSDF_ERR_CAPACITY;
  }
  if (total == 0) return 0;
  SIDE_CHECK_ARG(offsets != nullptr && aligned_to(offsets, 8));
  SIDE_CHECK_ARG(verts != nullptr && aligned_to(verts, 4) && keys != nullptr && aligned_to(keys, 8));
  SIDE_CHECK_ARG(aligned_to(colors, 4) && (const void*)verts != (const void*)keys && colors != verts &&
                 (const void*)colors != (const void*)keys);
  for (const void* out : {(const void*)verts, (const void*)keys, (const void*)colors})
    if (out) SIDE_CHECK_ARG(out != tsdf && out != weight && out != color && out != offsets);
  const Lattice L = {nx, ny, nz, ox, oy, oz, voxel};
  const int grid = (int)((cells + TSDF_THREADS - 1) / TSDF_THREADS);
  hipLaunchKernelGGL(k_mesh_emit, dim3(grid), dim3(TSDF_THREADS), 0, (hipStream_t)stream, L, cells, tsdf, weight, color,
                     min_weight, offsets, total, verts, keys, colors);
  SIDE_HIP(hipGetLastError());
  return 0;
}
