// Bilateral-grid appearance compensation for gfx950 (include/egs_bilagrid.h has the contract, DESIGN §3.15 the design).
//
// slice:      out(x, y) = A(gx, gy, gz(rgb)) [rgb, 1], A = the grid of 3 x 4 affine transforms read trilinearly
// slice_bwd:  dimage (written) and dgrid (accumulated into) of the same
// tv:         weight TV(G) and its gradient, one workgroup
//
// One workgroup owns BW x BH = 64 x 32 pixels: wave w takes the rows w, w + 4, .. of the block, lane l the column l, so a
// wave-instruction reads 256 contiguous bytes of a colour plane.  The pixels of a block touch a box of lattice nodes
// [cx0 .. cx0 + nx) x [cy0 .. cy0 + ny) x L.  largest_box() sizes the largest box of the launch on the host:
//
//   LDS path     the box fits LDS_FLOATS floats (32 KiB): the forward stages the box of G in LDS (12 floats per node,
//                three ds_read_b128 per corner); the backward stages G for dimage and sums the block's dgrid in a second
//                LDS box, which it flushes with ONE global float atomic per non-zero entry.  Inside the block:
//                  - boxes at most two columns wide and at most 8 layers (1080p with 16 x 16 x 8: every block): the
//                    matrix form, MFMAs that keep a wave's sums in registers across its rows (see k_slice_bwd);
//                  - otherwise a wave whose 64 pixels share one cell (same x0, z0; y0 is the wave's by construction)
//                    sums each of the 96 contributions across its lanes in registers (DPP) and issues one conflict-free
//                    LDS add per 64 sums, and in any other wave every lane adds its own (ds_add_f32: about 200 cycles
//                    per wave-instruction, measured).
//   global path  the box does not fit (cells smaller than pixels): G is read from global memory and dgrid takes
//                8 x 12 global float atomics per pixel.
//
// out and dimage involve no atomics and are bitwise reproducible; dgrid is a float-atomic sum and is not.
//
// Lattice coordinates: gx = float(x (Gw - 1)) / float(max(W - 1, 1)).  The product is below 2^22 (checked), so it is exact
// in float32 and the floor of the correctly rounded quotient is the integer quotient: a pixel's cell is the one the host's
// integer arithmetic (and appearance.slice_path) gives, and a block's box is spanned by its first and last pixel.
#define EGS_SIDE_LIBRARY "egs_bilagrid"
#include "egs_side_error.h"
#include "../../include/egs_bilagrid.h"

namespace egs_bilagrid {

using namespace egs;

constexpr int BW = EGS_BILAGRID_BLOCK_W, BH = EGS_BILAGRID_BLOCK_H, THREADS = 256, WAVES = THREADS / 64;
constexpr int LDS_FLOATS = EGS_BILAGRID_LDS_FLOATS;
constexpr int TV_THREADS = 1024;
static_assert(BW == 64, "one lane per column of the block");
static_assert(2 * LDS_FLOATS * sizeof(float) <= 65536, "G and dG boxes of the backward pass: one launch's LDS");

struct Params {
  int H, W, Gw, Gh, L;
  int denx, deny;      // max(W - 1, 1), max(H - 1, 1)
  const float* image;
  const float* grid;
  const float* dout;
  float* out;
  float* dimage;
  float* dgrid;
};

// lower node of the cell of coordinate num / den on an axis of g nodes, and the position inside the cell (1 at the last
// node of the axis; 0 on an axis of one node)
__host__ __device__ inline int cell_of(int num, int den, int g) {
  const int c = num / den;
  return c < g - 2 ? c : (g - 2 > 0 ? g - 2 : 0);
}
__device__ __forceinline__ int cell_f(int num, int den, int g, float& frac) {
  const float q = (float)num / (float)den;
  int c = (int)q;                                   // q >= 0: truncation is the floor
  const int top = g - 2 > 0 ? g - 2 : 0;
  c = c < top ? c : top;
  frac = q - (float)c;
  return c;
}
__host__ __device__ inline int upper(int c, int g) { return c + 1 < g ? c + 1 : g - 1; }

// the box of nodes of the pixels [p0, p1] of an axis: first node and node count
__host__ __device__ inline void span_of(int p0, int p1, int scale, int den, int g, int& c0, int& n) {
  c0 = cell_of(p0 * scale, den, g);
  n = upper(cell_of(p1 * scale, den, g), g) - c0 + 1;
}

// 12 floats of one node: LDS box (node = index in the box, 12 contiguous floats) or global grid (node = index in one
// channel plane of cs floats)
template <bool LDS>
__device__ __forceinline__ void load12(const float* __restrict__ src, int node, int cs, float a[12]) {
  if (LDS) {
    const float4* s = (const float4*)(src + node * 12);
    const float4 u = s[0], v = s[1], w = s[2];
    a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w; a[4] = v.x; a[5] = v.y; a[6] = v.z; a[7] = v.w;
    a[8] = w.x; a[9] = w.y; a[10] = w.z; a[11] = w.w;
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) a[k] = src[(size_t)k * cs + node];
  }
}

// where a pixel reads the lattice: four (x, y) node indices (in the box or in a plane) for the layers z0 and z1, and the
// three positions inside the cell
struct Taps {
  int n00, n01, n10, n11;   // (y0,x0) (y0,x1) (y1,x0) (y1,x1) on layer z0
  int dz;                   // + dz: the same on layer z1 (0 when L == 1)
  int z0, rx0, rx1, ry0, ry1;   // LDS path: the layer and the box columns / rows behind the four indices
  float fx, fy, fz;
  float luma;
};

// the affine transform at the taps: A and, for the guidance term, dA = A_xy(z1) - A_xy(z0)
template <bool LDS>
__device__ __forceinline__ void interpolate(const float* __restrict__ src, const Taps& t, int cs, float A[12],
                                            float dA[12]) {
  const float w00 = (1.f - t.fx) * (1.f - t.fy), w01 = t.fx * (1.f - t.fy), w10 = (1.f - t.fx) * t.fy, w11 = t.fx * t.fy;
  float a[12], b0[12];
  load12<LDS>(src, t.n00, cs, a);
#pragma unroll
  for (int k = 0; k < 12; ++k) b0[k] = w00 * a[k];
  load12<LDS>(src, t.n01, cs, a);
#pragma unroll
  for (int k = 0; k < 12; ++k) b0[k] = __builtin_fmaf(w01, a[k], b0[k]);
  load12<LDS>(src, t.n10, cs, a);
#pragma unroll
  for (int k = 0; k < 12; ++k) b0[k] = __builtin_fmaf(w10, a[k], b0[k]);
  load12<LDS>(src, t.n11, cs, a);
#pragma unroll
  for (int k = 0; k < 12; ++k) b0[k] = __builtin_fmaf(w11, a[k], b0[k]);
  load12<LDS>(src, t.n00 + t.dz, cs, a);
#pragma unroll
  for (int k = 0; k < 12; ++k) dA[k] = w00 * a[k];
  load12<LDS>(src, t.n01 + t.dz, cs, a);
#pragma unroll
  for (int k = 0; k < 12; ++k) dA[k] = __builtin_fmaf(w01, a[k], dA[k]);
  load12<LDS>(src, t.n10 + t.dz, cs, a);
#pragma unroll
  for (int k = 0; k < 12; ++k) dA[k] = __builtin_fmaf(w10, a[k], dA[k]);
  load12<LDS>(src, t.n11 + t.dz, cs, a);
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    dA[k] = __builtin_fmaf(w11, a[k], dA[k]) - b0[k];
    A[k] = __builtin_fmaf(t.fz, dA[k], b0[k]);
  }
}

// What a workgroup knows about its block: pixel range, box of nodes, and this lane's column
struct Block {
  int px0, py0, rows;       // first pixel, rows of the block inside the image
  int cx0, cy0, nx, ny;     // the box
  int x;                    // this lane's column, clamped into the image
  bool live;                // .. and whether it is a pixel of the image
  int x0, x1;               // the column's two nodes, absolute
  float fx;
};

__device__ __forceinline__ Block block_of(const Params& p) {
  Block b;
  b.px0 = blockIdx.x * BW;
  b.py0 = blockIdx.y * BH;
  const int px1 = min(b.px0 + BW, p.W) - 1, py1 = min(b.py0 + BH, p.H) - 1;
  b.rows = py1 - b.py0 + 1;
  span_of(b.px0, px1, p.Gw - 1, p.denx, p.Gw, b.cx0, b.nx);
  span_of(b.py0, py1, p.Gh - 1, p.deny, p.Gh, b.cy0, b.ny);
  const int x = b.px0 + (threadIdx.x & 63);
  b.live = x < p.W;
  b.x = b.live ? x : p.W - 1;
  b.x0 = cell_f(b.x * (p.Gw - 1), p.denx, p.Gw, b.fx);
  b.x1 = upper(b.x0, p.Gw);
  return b;
}

// the taps of pixel (b.x, y) with colour (r, g, bl)
template <bool LDS>
__device__ __forceinline__ Taps taps_of(const Params& p, const Block& b, int y, float r, float g, float bl) {
  Taps t;
  t.fx = b.fx;
  const int y0 = cell_f(y * (p.Gh - 1), p.deny, p.Gh, t.fy);
  const int y1 = upper(y0, p.Gh);
  t.luma = 0.299f * r + 0.587f * g + 0.114f * bl;
  const float gz = fminf(fmaxf(t.luma, 0.f), 1.f) * (float)(p.L - 1);
  int z0 = (int)gz;
  const int top = p.L - 2 > 0 ? p.L - 2 : 0;
  z0 = z0 < top ? z0 : top;
  t.fz = gz - (float)z0;
  if (LDS) {
    // (the clamps hold by construction -- span_of covers the block's first and last pixel -- and cost two v_med3 each)
    const int rx0 = min(max(b.x0 - b.cx0, 0), b.nx - 1), rx1 = min(max(b.x1 - b.cx0, 0), b.nx - 1);
    const int ry0 = min(max(y0 - b.cy0, 0), b.ny - 1), ry1 = min(max(y1 - b.cy0, 0), b.ny - 1);
    const int base = z0 * b.ny;
    t.n00 = (base + ry0) * b.nx + rx0; t.n01 = (base + ry0) * b.nx + rx1;
    t.n10 = (base + ry1) * b.nx + rx0; t.n11 = (base + ry1) * b.nx + rx1;
    t.dz = p.L > 1 ? b.ny * b.nx : 0;
    t.z0 = z0; t.rx0 = rx0; t.rx1 = rx1; t.ry0 = ry0; t.ry1 = ry1;
  } else {
    const int base = z0 * p.Gh;
    t.n00 = (base + y0) * p.Gw + b.x0; t.n01 = (base + y0) * p.Gw + b.x1;
    t.n10 = (base + y1) * p.Gw + b.x0; t.n11 = (base + y1) * p.Gw + b.x1;
    t.dz = p.L > 1 ? p.Gh * p.Gw : 0;
  }
  return t;
}

// box entry e, counted in the grid's own order (channel, layer, row, column: neighbouring lanes read and add to
// neighbouring addresses of a grid row) -> its place in the LDS box and in the grid
__device__ __forceinline__ void box_entry(const Params& p, const Block& b, int e, int& lds, size_t& glob) {
  const int xx = e % b.nx;
  int r = e / b.nx;
  const int yy = r % b.ny;
  r /= b.ny;
  const int z = r % p.L, ch = r / p.L;
  lds = ((z * b.ny + yy) * b.nx + xx) * 12 + ch;
  glob = (((size_t)ch * p.L + z) * p.Gh + (b.cy0 + yy)) * p.Gw + (b.cx0 + xx);
}

template <bool LDS>
__global__ __launch_bounds__(THREADS) void k_slice(Params p) {
  extern __shared__ float4 smem4[];
  float* sG = (float*)smem4;
  const Block b = block_of(p);
  const int cs = p.L * p.Gh * p.Gw;
  if (LDS) {
    const int count = b.nx * b.ny * p.L * 12;
    for (int e = threadIdx.x; e < count; e += THREADS) {
      int lds;
      size_t glob;
      box_entry(p, b, e, lds, glob);
      sG[lds] = p.grid[glob];
    }
    __syncthreads();
  }
  if (!b.live) return;
  const float* src = LDS ? sG : p.grid;
  const size_t plane = (size_t)p.H * p.W;
  for (int r = threadIdx.x >> 6; r < b.rows; r += WAVES) {
    const int y = b.py0 + r;
    const size_t at = (size_t)y * p.W + b.x;
    const float cr = p.image[at], cg = p.image[plane + at], cb = p.image[2 * plane + at];
    const Taps t = taps_of<LDS>(p, b, y, cr, cg, cb);
    float A[12], dA[12];
    interpolate<LDS>(src, t, cs, A, dA);
    p.out[at] = __builtin_fmaf(A[0], cr, __builtin_fmaf(A[1], cg, __builtin_fmaf(A[2], cb, A[3])));
    p.out[plane + at] = __builtin_fmaf(A[4], cr, __builtin_fmaf(A[5], cg, __builtin_fmaf(A[6], cb, A[7])));
    p.out[2 * plane + at] = __builtin_fmaf(A[8], cr, __builtin_fmaf(A[9], cg, __builtin_fmaf(A[10], cb, A[11])));
  }
}

template <int CTRL>
__device__ __forceinline__ float dpp_read(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// the sum of v over the 64 lanes of a wave whose lanes are ALL active: quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror and row_mirror leave every lane with the sum of its row of 16; the four rows meet in scalars
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_read<0xB1>(v);
  v += dpp_read<0x4E>(v);
  v += dpp_read<0x141>(v);
  v += dpp_read<0x140>(v);
  const int i = __float_as_int(v);
  return (__int_as_float(__builtin_amdgcn_readlane(i, 0)) + __int_as_float(__builtin_amdgcn_readlane(i, 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(i, 32)) + __int_as_float(__builtin_amdgcn_readlane(i, 48)));
}

// The matrix form of the dgrid sum (MAT; the host picks it when every block's box is at most MAT_NX = 2 columns wide and
// the grid has at most MAT_L = 8 layers).  Along a row of 64 pixels y0, y1 and fy are the wave's, so the row's share of
// dgrid is a matrix product: S[node][ch] = sum_pixel Wt[node][pixel] V[pixel][ch], node = 2 z + column (16 of them),
// V[pixel][4c + j] = dout_c [rgb, 1]_j, and Wt holds each pixel's four weights wz wx.  Sixteen
// v_mfma_f32_16x16x4_f32 per accumulator sum a row (k = 4 pixels each); the two accumulators, for the node rows y0 and
// y1, carry (1 - fy) Wt and fy Wt and live in registers across the wave's rows until y0 changes.  Then each is added to
// the LDS box once: 8 conflict-free LDS adds instead of 96 contended ones per row.
// The operands cross lanes through a per-wave LDS scratch: lane l of MFMA g holds pixel 16 (l >> 4) + g in its k slot.
constexpr int MAT_NX = 2, MAT_L = 8;
constexpr int MAT_V = 12, MAT_W = 4;                            // floats per pixel: V row; the four weights
constexpr int MAT_WAVE_FLOATS = 64 * (MAT_V + MAT_W + 1);       // .. and the four node indices, packed
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void mat_flush(float* sD, const f32x4& acc, int ry, int nx, int ny, int L) {
  const int j = threadIdx.x & 15, i0 = ((threadIdx.x & 63) >> 4) * 4;        // C[i0 + r][j] in register r
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int z = (i0 + r) >> 1, xc = (i0 + r) & 1;
    if (j < 12 && z < L && xc < nx && acc[r] != 0.f) atomicAdd(&sD[((z * ny + ry) * nx + xc) * 12 + j], acc[r]);
  }
}

// DIMG / DGRID: which halves the caller wants.  Every lane of a wave stays active through the row loop (a column outside
// the image reads the image's last column and carries dout = 0), so wave_sum and the MFMAs see a full wave.
template <bool LDS, bool DIMG, bool DGRID, bool MAT>
__global__ __launch_bounds__(THREADS) void k_slice_bwd(Params p) {
  static_assert(!MAT || (LDS && DGRID), "the matrix form accumulates into the LDS box");
  extern __shared__ float4 smem4[];
  const Block b = block_of(p);
  const int cs = p.L * p.Gh * p.Gw;
  const int count = b.nx * b.ny * p.L * 12;
  float* sG = (float*)smem4;                                   // the box of G (DIMG)
  float* sD = (float*)smem4 + (DIMG ? count : 0);              // the box of dG (DGRID); count is a multiple of 4
  float* sV = sD + count + (threadIdx.x >> 6) * MAT_WAVE_FLOATS;   // this wave's scratch (MAT): V rows,
  float4* sW = (float4*)(sV + 64 * MAT_V);                         // weights,
  int* sN = (int*)(sV + 64 * (MAT_V + MAT_W));                     // node indices
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int acc_ry0 = -1, acc_ry1 = -1;                                  // the node rows the accumulators belong to
  if (LDS) {
    for (int e = threadIdx.x; e < count; e += THREADS) {
      if (DIMG) {
        int lds;
        size_t glob;
        box_entry(p, b, e, lds, glob);
        sG[lds] = p.grid[glob];
      }
      if (DGRID) sD[e] = 0.f;
    }
    __syncthreads();
  }
  const float* src = LDS ? sG : p.grid;
  const size_t plane = (size_t)p.H * p.W;
  const int lane = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < b.rows; r += WAVES) {
    const int y = b.py0 + r;
    const size_t at = (size_t)y * p.W + b.x;
    const float rgb1[4] = {p.image[at], p.image[plane + at], p.image[2 * plane + at], 1.f};
    float d[3] = {p.dout[at], p.dout[plane + at], p.dout[2 * plane + at]};
    if (!b.live) d[0] = d[1] = d[2] = 0.f;
    const Taps t = taps_of<LDS>(p, b, y, rgb1[0], rgb1[1], rgb1[2]);
    if (DIMG) {
      float A[12], dA[12];
      interpolate<LDS>(src, t, cs, A, dA);
      float g[3], through = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) g[j] = A[j] * d[0] + A[4 + j] * d[1] + A[8 + j] * d[2];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        through += d[c] * (dA[4 * c] * rgb1[0] + dA[4 * c + 1] * rgb1[1] + dA[4 * c + 2] * rgb1[2] + dA[4 * c + 3]);
      if (p.L > 1 && t.luma > 0.f && t.luma < 1.f) {
        through *= (float)(p.L - 1);
        g[0] = __builtin_fmaf(0.299f, through, g[0]);
        g[1] = __builtin_fmaf(0.587f, through, g[1]);
        g[2] = __builtin_fmaf(0.114f, through, g[2]);
      }
      if (b.live) {
        p.dimage[at] = g[0]; p.dimage[plane + at] = g[1]; p.dimage[2 * plane + at] = g[2];
      }
    }
    if (DGRID) {
      float v[12];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * c + j] = d[c] * rgb1[j];
      const float wx[2] = {1.f - t.fx, t.fx}, wy[2] = {1.f - t.fy, t.fy}, wz[2] = {1.f - t.fz, t.fz};
      const int node[4] = {t.n00, t.n01, t.n10, t.n11};
      if (MAT) {
        // this pixel's row of V, its four weights and their nodes (2 z + column)
        const int z0 = t.z0, z1 = z0 + (t.dz ? 1 : 0), rx0 = t.rx0, rx1 = t.rx1;
        const int ry0 = __builtin_amdgcn_readfirstlane(t.ry0), ry1 = __builtin_amdgcn_readfirstlane(t.ry1);
        if (ry0 != acc_ry0 || ry1 != acc_ry1) {                  // (wave-uniform) the wave moved to another row of cells
          if (acc_ry0 >= 0) {
            mat_flush(sD, acc0, acc_ry0, b.nx, b.ny, p.L);
            mat_flush(sD, acc1, acc_ry1, b.nx, b.ny, p.L);
          }
          acc0 = f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
          acc_ry0 = ry0; acc_ry1 = ry1;
        }
        float4* vrow = (float4*)(sV + lane * MAT_V);
        vrow[0] = make_float4(v[0], v[1], v[2], v[3]);
        vrow[1] = make_float4(v[4], v[5], v[6], v[7]);
        vrow[2] = make_float4(v[8], v[9], v[10], v[11]);
        sW[lane] = make_float4(wz[0] * wx[0], wz[0] * wx[1], wz[1] * wx[0], wz[1] * wx[1]);
        sN[lane] = (2 * z0 + rx0) | ((2 * z0 + rx1) << 8) | ((2 * z1 + rx0) << 16) | ((2 * z1 + rx1) << 24);
        __builtin_amdgcn_wave_barrier();                         // (one wave, LDS in order: its own writes are visible)
        const int i = lane & 15, first = lane & 48;
#pragma unroll 4
        for (int g = 0; g < 16; ++g) {
          const int px = first + g;
          const float4 w = sW[px];
          const int n = sN[px];
          const float bv = i < 12 ? sV[px * MAT_V + i] : 0.f;
          const float a = (i == (n & 255) ? w.x : 0.f) + (i == ((n >> 8) & 255) ? w.y : 0.f) +
                          (i == ((n >> 16) & 255) ? w.z : 0.f) + (i == ((n >> 24) & 255) ? w.w : 0.f);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a * wy[0], bv, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a * wy[1], bv, acc1, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
        continue;
      }
      if (LDS) {
        // one cell for the whole wave?  (n00 holds x0, y0 and z0; y0 is the wave's already)
        const bool uniform = __all(t.n00 == __builtin_amdgcn_readfirstlane(t.n00)) != 0;
        if (uniform) {
          // lane q of the first add holds corner q / 12, channel q % 12 (corners 0 .. 4, the fifth in part); lane q of
          // the second the remaining 32 sums
          float first = 0.f, second = 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float w = wz[k >> 2] * wy[(k >> 1) & 1] * wx[k & 1];
#pragma unroll
            for (int ch = 0; ch < 12; ++ch) {
              const float s = wave_sum(w * v[ch]);
              const int q = k * 12 + ch;
              if (q < 64) first = lane == q ? s : first;
              else second = lane == q - 64 ? s : second;
            }
          }
          const int k1 = lane / 12, k2 = (lane + 64) / 12;         // the corner of this lane's sum, then its node
          const int n1 = node[0] + ((k1 & 1) ? node[1] - node[0] : 0) + ((k1 & 2) ? node[2] - node[0] : 0) +
                         ((k1 & 4) ? t.dz : 0);
          const int n2 = node[0] + ((k2 & 1) ? node[1] - node[0] : 0) + ((k2 & 2) ? node[2] - node[0] : 0) +
                         ((k2 & 4) ? t.dz : 0);
          if (first != 0.f) atomicAdd(&sD[n1 * 12 + lane % 12], first);
          if (lane < 32 && second != 0.f) atomicAdd(&sD[n2 * 12 + (lane + 64) % 12], second);
          continue;
        }
      }
      if (!b.live) continue;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float w = wz[k >> 2] * wy[(k >> 1) & 1] * wx[k & 1];
        if (w == 0.f) continue;
        const int n = node[k & 3] + ((k & 4) ? t.dz : 0);
#pragma unroll
        for (int ch = 0; ch < 12; ++ch) {
          if (LDS) atomicAdd(&sD[n * 12 + ch], w * v[ch]);
          else atomicAdd(&p.dgrid[(size_t)ch * cs + n], w * v[ch]);
        }
      }
    }
  }
  if (MAT && acc_ry0 >= 0) {
    mat_flush(sD, acc0, acc_ry0, b.nx, b.ny, p.L);
    mat_flush(sD, acc1, acc_ry1, b.nx, b.ny, p.L);
  }
  if (LDS && DGRID) {
    __syncthreads();
    for (int e = threadIdx.x; e < count; e += THREADS) {
      int lds;
      size_t glob;
      box_entry(p, b, e, lds, glob);
      const float s = sD[lds];
      if (s != 0.f) atomicAdd(&p.dgrid[glob], s);
    }
  }
}

// TV and its gradient by ONE workgroup (a grid is a few ten thousand floats; a second launch to add partial sums would
// cost more than the loop).  Element i takes its own share of the gradient from its two neighbours along each axis: no
// atomics.  inv[a] = 1 / (number of forward differences along axis a), 0 for an axis of one node.
__global__ __launch_bounds__(TV_THREADS) void k_tv(int Gw, int Gh, int L, const float* __restrict__ G, float weight,
                                                   float ix, float iy, float iz, float* value_out,
                                                   float* __restrict__ dgrid) {
  __shared__ float part[TV_THREADS / 64];
  const int n = 12 * L * Gh * Gw;
  const int sy = Gw, sz = Gw * Gh;
  float sum = 0.f;
  for (int i = threadIdx.x; i < n; i += TV_THREADS) {
    const int x = i % Gw, y = (i / Gw) % Gh, z = (i / sz) % L;
    const float g = G[i];
    float grad = 0.f;
    if (x + 1 < Gw) { const float d = G[i + 1] - g; sum = __builtin_fmaf(d * d, ix, sum); grad -= ix * d; }
    if (x > 0) grad += ix * (g - G[i - 1]);
    if (y + 1 < Gh) { const float d = G[i + sy] - g; sum = __builtin_fmaf(d * d, iy, sum); grad -= iy * d; }
    if (y > 0) grad += iy * (g - G[i - sy]);
    if (z + 1 < L) { const float d = G[i + sz] - g; sum = __builtin_fmaf(d * d, iz, sum); grad -= iz * d; }
    if (z > 0) grad += iz * (g - G[i - sz]);
    if (dgrid) dgrid[i] += 2.f * weight * grad;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int k = 0; k < TV_THREADS / 64; ++k) s += part[k];
    *value_out = weight * s;
  }
}

// the largest box of a launch, in floats (the host's half of the path decision; appearance.slice_path mirrors it), and
// its width in nodes
static int64_t largest_box(int H, int W, int Gw, int Gh, int L, int* widest = nullptr) {
  int nx = 1, ny = 1;
  for (int p0 = 0; p0 < W; p0 += BW) {
    int c0, n;
    span_of(p0, (p0 + BW < W ? p0 + BW : W) - 1, Gw - 1, W - 1 > 1 ? W - 1 : 1, Gw, c0, n);
    nx = n > nx ? n : nx;
  }
  for (int p0 = 0; p0 < H; p0 += BH) {
    int c0, n;
    span_of(p0, (p0 + BH < H ? p0 + BH : H) - 1, Gh - 1, H - 1 > 1 ? H - 1 : 1, Gh, c0, n);
    ny = n > ny ? n : ny;
  }
  if (widest) *widest = nx;
  return (int64_t)nx * ny * L * 12;
}

static int check_shape(int device, int H, int W, int Gw, int Gh, int L) {
  SIDE_CHECK_ARG(device >= 0);
  SIDE_CHECK_ARG(H > 0 && W > 0);
  SIDE_CHECK_ARG(Gw > 0 && Gh > 0 && L > 0);
  SIDE_CHECK_ARG((int64_t)Gw * Gh * L * 12 <= EGS_BILAGRID_MAX_GRID_FLOATS);
  SIDE_CHECK_ARG((int64_t)(W - 1) * (Gw - 1) < EGS_BILAGRID_MAX_COORD_PRODUCT);
  SIDE_CHECK_ARG((int64_t)(H - 1) * (Gh - 1) < EGS_BILAGRID_MAX_COORD_PRODUCT);
  SIDE_CHECK_ARG((int64_t)H * W <= ((int64_t)1 << 28));
  SIDE_CHECK_ARG((H + BH - 1) / BH <= 65535);
  return 0;
}

static bool aligned4(const void* a) { return ((uintptr_t)a & 3) == 0; }

static Params fill(int H, int W, int Gw, int Gh, int L, const float* image, const float* grid) {
  Params p;
  p.H = H; p.W = W; p.Gw = Gw; p.Gh = Gh; p.L = L;
  p.denx = W - 1 > 1 ? W - 1 : 1;
  p.deny = H - 1 > 1 ? H - 1 : 1;
  p.image = image; p.grid = grid;
  p.dout = nullptr; p.out = nullptr; p.dimage = nullptr; p.dgrid = nullptr;
  return p;
}

// run `launch` with `device` current, then restore the caller's device
template <class F>
static int on_device(int device, F launch) {
  int before = 0;
  SIDE_HIP(hipGetDevice(&before));
  if (before != device) SIDE_HIP(hipSetDevice(device));
  launch();
  const hipError_t e = hipGetLastError();
  if (before != device) SIDE_HIP(hipSetDevice(before));
  SIDE_HIP(e);
  return 0;
}

}  // namespace egs_bilagrid

using namespace egs_bilagrid;

extern "C" int egs_bilagrid_abi_version(void) { return EGS_BILAGRID_ABI_VERSION; }
extern "C" const char* egs_bilagrid_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_bilagrid_slice(int device, void* stream, int H, int W, int Gw, int Gh, int L, const float* image,
                                  const float* grid, float* out) {
  if (int rc = check_shape(device, H, W, Gw, Gh, L)) return rc;
  SIDE_CHECK_ARG(image != nullptr && aligned4(image));
  SIDE_CHECK_ARG(grid != nullptr && aligned4(grid));
  SIDE_CHECK_ARG(out != nullptr && aligned4(out) && out != image);
  Params p = fill(H, W, Gw, Gh, L, image, grid);
  p.out = out;
  const int64_t box = largest_box(H, W, Gw, Gh, L);
  const dim3 blocks(div_up(W, BW), div_up(H, BH));
  return on_device(device, [&] {
    if (box <= LDS_FLOATS)
      hipLaunchKernelGGL(k_slice<true>, blocks, dim3(THREADS), (size_t)box * sizeof(float), (hipStream_t)stream, p);
    else
      hipLaunchKernelGGL(k_slice<false>, blocks, dim3(THREADS), 0, (hipStream_t)stream, p);
  });
}

extern "C" int egs_bilagrid_slice_bwd(int device, void* stream, int H, int W, int Gw, int Gh, int L,
                                      const float* image, const float* grid, const float* dout, float* dimage,
                                      float* dgrid) {
  if (int rc = check_shape(device, H, W, Gw, Gh, L)) return rc;
  SIDE_CHECK_ARG(image != nullptr && aligned4(image));
  SIDE_CHECK_ARG(grid != nullptr && aligned4(grid));
  SIDE_CHECK_ARG(dout != nullptr && aligned4(dout));
  SIDE_CHECK_ARG(aligned4(dimage) && aligned4(dgrid));
  SIDE_CHECK_ARG(dimage == nullptr || (dimage != image && dimage != dout));
  if (!dimage && !dgrid) return 0;
  Params p = fill(H, W, Gw, Gh, L, image, grid);
  p.dout = dout; p.dimage = dimage; p.dgrid = dgrid;
  int widest = 0;
  const int64_t box = largest_box(H, W, Gw, Gh, L, &widest);
  const bool lds = box <= LDS_FLOATS;
  const bool mat = lds && dgrid && widest <= MAT_NX && L <= MAT_L;
  const dim3 blocks(div_up(W, BW), div_up(H, BH));
  const size_t bytes = lds ? sizeof(float) * ((size_t)box * ((dimage ? 1 : 0) + (dgrid ? 1 : 0)) +
                                              (mat ? WAVES * MAT_WAVE_FLOATS : 0)) : 0;
  decltype(&k_slice_bwd<true, true, true, false>) kern;
  if (mat) kern = dimage ? k_slice_bwd<true, true, true, true> : k_slice_bwd<true, false, true, true>;
  else if (lds) kern = dimage && dgrid ? k_slice_bwd<true, true, true, false>
                       : dimage ? k_slice_bwd<true, true, false, false> : k_slice_bwd<true, false, true, false>;
  else kern = dimage && dgrid ? k_slice_bwd<false, true, true, false>
              : dimage ? k_slice_bwd<false, true, false, false> : k_slice_bwd<false, false, true, false>;
  return on_device(device, [&] { hipLaunchKernelGGL(kern, blocks, dim3(THREADS), bytes, (hipStream_t)stream, p); });
}

extern "C" int egs_bilagrid_tv(int device, void* stream, int Gw, int Gh, int L, const float* grid, float weight,
                               float* value_out, float* dgrid) {
  if (int rc = check_shape(device, 1, 1, Gw, Gh, L)) return rc;
  SIDE_CHECK_ARG(grid != nullptr && aligned4(grid));
  SIDE_CHECK_ARG(value_out != nullptr && aligned4(value_out));
  SIDE_CHECK_ARG(aligned4(dgrid) && dgrid != grid);
  const double per = 12.0 * L * Gh * Gw;
  const float ix = Gw > 1 ? (float)(1.0 / (per / Gw * (Gw - 1))) : 0.f;
  const float iy = Gh > 1 ? (float)(1.0 / (per / Gh * (Gh - 1))) : 0.f;
  const float iz = L > 1 ? (float)(1.0 / (per / L * (L - 1))) : 0.f;
  return on_device(device, [&] {
    hipLaunchKernelGGL(k_tv, dim3(1), dim3(TV_THREADS), 0, (hipStream_t)stream, Gw, Gh, L, grid, weight, ix, iy, iz,
                       value_out, dgrid);
  });
}
