// Fused training loss for gfx950: gau_loss = (1-lambda) * L1 + lambda * (1 - SSIM)
// (reference gsplat/pytorch_ssim.py:10-66: five depthwise 11x11 Gaussian-window conv2d
// calls forward plus their autograd backward in PyTorch -- measured 10.9 ms per 1920x1080
// image on MI355X).  Here: two tiled kernels, separable 11-tap window staged in LDS,
// producing the loss AND dL/dimage (the input of splatB) directly.
//
// This header is the only text of that device code, and of the host side of a launch (window, grid, workspace): one
// forward body and one gradient body with a `bool WEIGHTED` parameter, wrapped in __global__ kernels by the source file
// that launches them.  Every weighted statement sits behind `if constexpr (WEIGHTED)`.
//   <false> : k_ssim_fwd, k_ssim_bwd, k_loss_finalize of egs_loss.hip (libegs_hip.so: egs_gau_loss, every pixel counts
//             once; the weighted arguments are nullptr / 0);
//   <true>  : k_ssim_fwd_w, k_ssim_bwd_w, k_loss_finalize_w of egs_wloss.hip (libegs_wloss.so: egs_wloss, a weight per
//             pixel).
// Where a sum of two products leaves the compiler the choice of which one to fuse, the fused form is written out
// (__builtin_fmaf), so that both instances round alike whatever is compiled around them: w == 1 gives the bits of
// egs_gau_loss (tests/test_gpu_weighted_loss.py).
//
//   ssim_fwd_body : per 64x16 tile and channel: mu1, mu2, E[x^2], E[y^2], E[xy] -> SSIM map value,
//                   per-tile partial sums of |x-y| and SSIM, and the three partial-derivative
//                   maps Pm = dS/dmu1, P11 = dS/dE11, P12 = dS/dE12.
//   ssim_bwd_body : dS_total/dx = W*Pm + 2x (W*P11) + y (W*P12)   (W symmetric, zero padding),
//                   dL/dx = (1-lambda)/M sign(x-y) - lambda/M dS_total/dx.
//   loss_finalize : deterministic reduction of the per-tile partials.
//
// WEIGHTED: w [H][W] >= 0, one plane for the three channels.  The SSIM map is that of the UNWEIGHTED
// images; the forward body stores w Pm, w P11, w P12, sums w |x-y| and w S, and leaves sum(w) of every channel-0 tile
// in `wparts`; the gradient body reduces `wparts` in every workgroup (fixed order, no atomics: the same bits everywhere)
// and takes M = 3 sum(w) from it, so the host never reads the sum.
//
// 275 MB of HBM traffic per 1080p image (x,y in; 3 maps out; 3 maps + x,y in; grad out); the window
// passes are what costs: both are register-blocked (a thread slides the 11 taps over a run of 8 outputs of a
// row / 4 outputs of a column, reading every LDS value once per run instead of once per tap).
#pragma once
#include <math.h>

#include "egs_common.h"

namespace egs {

constexpr int LW = 11, LR = 5;            // window size / radius (pytorch_ssim.py:52: window_size=11)
constexpr int TW = 64, TH = 16;           // output tile
constexpr int IW = TW + 2 * LR, IH = TH + 2 * LR;  // input tile with halo: 74 x 26
constexpr int HRUN = 8, VRUN = 4;         // outputs per thread: horizontal pass (row run), vertical pass (column run)
constexpr int HSEG = TW / HRUN;           // 8 runs per tile row -> IH * HSEG = 208 of the 256 threads work
constexpr int NLOAD = (IH * IW + 255) / 256;  // halo-tile elements per thread
static_assert(IH * HSEG <= 256 && TW * (TH / VRUN) == 256, "pass shapes are tied to the 256-thread workgroup");

struct LossWin { float g[LW]; };          // normalised 1-D Gaussian, sigma = 1.5 (pytorch_ssim.py:11-13,17)

// ---- host side of a launch: the window, the tile count, the persistent grid, the workspace -------------------------
static inline LossWin loss_window() {
  LossWin win;
  double sum = 0.0, g[LW];
  for (int i = 0; i < LW; ++i) { g[i] = exp(-(double)((i - LR) * (i - LR)) / (2.0 * 1.5 * 1.5)); sum += g[i]; }
  for (int i = 0; i < LW; ++i) win.g[i] = (float)(g[i] / sum);
  return win;
}
static inline int loss_blocks(int H, int W) { return div_up(W, TW) * div_up(H, TH) * 3; }
static inline int loss_grid(int nb) {
  static const int resident = [] {  // persistent workgroups: 3 per CU (LDS), every CU of the current device
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    return 3 * cus;
  }();
  return nb < resident ? nb : resident;
}
// The workspace of a call, 256-B aligned pieces: the three derivative maps [3][H][W], the per-tile partials [nb][2] and,
// for the weighted call, sum(w) of the channel-0 tiles [nb / 3].  `bytes` is what the *_ws_bytes entry points report (a
// 256-B tail is part of it); ws == NULL asks for `bytes` alone.
struct LossWs { float *Pm, *P11, *P12, *partials, *wparts; size_t bytes; };
static inline LossWs loss_ws(void* ws, int H, int W, bool weighted) {
  const size_t nb = (size_t)loss_blocks(H, W);
  const size_t map = align_up((size_t)3 * H * W * 4, 256);
  const size_t o_parts = 3 * map, o_w = o_parts + align_up(nb * 8, 256);
  const size_t end = weighted ? o_w + align_up(nb / 3 * 4, 256) : o_w;
  auto at = [ws](size_t o) { return ws ? (float*)((char*)ws + o) : nullptr; };
  return {at(0), at(map), at(2 * map), at(o_parts), weighted ? at(o_w) : nullptr, end + 256};
}

#ifdef __HIPCC__
// image pixel (or 0: F.conv2d padding=5) of halo-tile element i
__device__ __forceinline__ bool tile_src(int i, int x0, int y0, int H, int W, int& r, int& c, size_t& off) {
  r = i / IW; c = i - r * IW;
  const int yy = y0 + r - LR, xx = x0 + c - LR;
  off = (size_t)yy * W + xx;
  return yy >= 0 && yy < H && xx >= 0 && xx < W;
}

// Persistent workgroups: a workgroup takes every step-th tile of its share (tile_walk); the halo tile of the NEXT tile is
// fetched into registers while the two window passes of the current one run, so the HBM latency is paid
// once per workgroup instead of once per tile (3 workgroups per CU fit: 49 KB of LDS each).
struct TileAt { int x0, y0; size_t plane; };
__device__ __forceinline__ TileAt tile_at(int t, int gx, int gy, int H, int W) {
  const int bx = t % gx, by = (t / gx) % gy, ch = t / (gx * gy);
  return {bx * TW, by * TH, (size_t)ch * H * W};
}

// Which tiles a persistent workgroup takes.  Workgroup b runs on XCD b % 8 (observed dispatch order; speed only), and
// every XCD has its own 4-MB L2: with tiles b, b + grid, ... the two tiles that share a halo column sit on different
// XCDs and the ones that share halo rows too (30 tiles per row, 30 % 8 != 0), so every halo came from HBM -- FETCH_SIZE
// read 155 MB for the forward kernel's 50 MB of pixels and 281 MB for the gradient kernel's 125 (rocprofv3 --pmc).
// Here every XCD walks a contiguous eighth of the tile list (row-major over channel, tile row, tile column), its
// resident workgroups side by side: the ~96 tiles in flight on an XCD span three tile rows (1.5 MB of halo tiles).
// (Eight XCDs and the b % 8 dispatch are MI355X's -- this library is built for gfx950 only, csrc/Makefile.  The walk is
// CORRECT for any mapping of workgroups to dies: on a part with another die count the bands would merely stop matching
// the L2s, i.e. fall back to what the strided walk did.)
struct TileWalk { int t, end, step; };
__device__ __forceinline__ TileWalk tile_walk(int ntiles) {
  const int b = blockIdx.x, G = gridDim.x;
  if (G < 16) return {b, ntiles, G};
  const int xcd = b & 7, slot = b >> 3;
  const int per = (G - xcd + 7) >> 3;                       // workgroups that run on this XCD
  const int lo = (int)((long long)ntiles * xcd / 8), hi = (int)((long long)ntiles * (xcd + 1) / 8);
  return {lo + slot, hi, per};
}

// WEIGHTED: `weight` [H][W] (NO channel plane offset), `wparts` [gx gy]: sum(w) of tile t < gx gy (channel 0: every
// pixel counts once).  Both unused otherwise.
template <bool WEIGHTED>
__device__ __forceinline__ void ssim_fwd_body(int H, int W, int gx, int gy, LossWin win,
                                              const float* __restrict__ img, const float* __restrict__ gt,
                                              float* __restrict__ Pm, float* __restrict__ P11,
                                              float* __restrict__ P12,
                                              float* __restrict__ partials /* [ntiles][2] */,
                                              const float* __restrict__ weight, float* __restrict__ wparts) {
  __shared__ float sx[IH][IW + 1], sy[IH][IW + 1];
  __shared__ float h[5][IH][TW + 1];      // horizontally filtered x, y, xx, yy, xy
  __shared__ float red[WEIGHTED ? 3 : 2][4];
  const int tid = threadIdx.x;
  const int ntiles = gx * gy * 3;
  float fa[NLOAD], fb[NLOAD];             // halo tile in flight: element tid + 256 j
  auto fetch = [&](int t) {               // every load is issued before anything waits on one
    const TileAt T = tile_at(t, gx, gy, H, W);
#pragma unroll
    for (int j = 0; j < NLOAD; ++j) {
      int r, c; size_t off;
      fa[j] = 0.f; fb[j] = 0.f;
      const int i = tid + 256 * j;
      if (i < IH * IW && tile_src(i, T.x0, T.y0, H, W, r, c, off)) { fa[j] = img[T.plane + off]; fb[j] = gt[T.plane + off]; }
    }
  };
  const TileWalk tw = tile_walk(ntiles);
  int t = tw.t;
  if (t < tw.end) fetch(t);
  for (; t < tw.end; t += tw.step) {
  const TileAt T = tile_at(t, gx, gy, H, W);
  const int x0 = T.x0, y0 = T.y0;
  const size_t plane = T.plane;
  float wv[VRUN];                         // this thread's VRUN weights: fetched first, consumed after both passes
  if constexpr (WEIGHTED) {
    const int oc = tid % TW, or0 = (tid / TW) * VRUN;
#pragma unroll
    for (int o = 0; o < VRUN; ++o) {
      const int yy = y0 + or0 + o, xx = x0 + oc;
      wv[o] = 0.f;
      if (yy < H && xx < W) wv[o] = weight[(size_t)yy * W + xx];
    }
  }
#pragma unroll
  for (int j = 0; j < NLOAD; ++j) {
    const int i = tid + 256 * j;
    if (i < IH * IW) { const int r = i / IW, c = i - r * IW; sx[r][c] = fa[j]; sy[r][c] = fb[j]; }
  }
  __syncthreads();
  if (t + tw.step < tw.end) fetch(t + tw.step);
  if (tid < IH * HSEG) {  // horizontal 11-tap pass: HRUN outputs of row r from HRUN + 10 inputs
    const int r = tid % IH, c0 = (tid / IH) * HRUN;  // lanes of a wave walk down the rows: odd row stride, few bank conflicts
    float u[HRUN + LW - 1], v[HRUN + LW - 1];
#pragma unroll
    for (int k = 0; k < HRUN + LW - 1; ++k) { u[k] = sx[r][c0 + k]; v[k] = sy[r][c0 + k]; }
    float a[HRUN], b[HRUN], aa[HRUN], bb[HRUN], ab[HRUN];
#pragma unroll
    for (int o = 0; o < HRUN; ++o) { a[o] = 0.f; b[o] = 0.f; aa[o] = 0.f; bb[o] = 0.f; ab[o] = 0.f; }
#pragma unroll
    for (int k = 0; k < HRUN + LW - 1; ++k) {
      const float uu = u[k] * u[k], vv = v[k] * v[k], uv = u[k] * v[k];
#pragma unroll
      for (int o = 0; o < HRUN; ++o) {
        const int tp = k - o;  // tap index of input k for output o (ascending k == ascending tap: the reference's order)
        if (tp >= 0 && tp < LW) {
          const float w = win.g[tp];
          a[o] += w * u[k]; b[o] += w * v[k]; aa[o] += w * uu; bb[o] += w * vv; ab[o] += w * uv;
        }
      }
    }
#pragma unroll
    for (int o = 0; o < HRUN; ++o) {
      h[0][r][c0 + o] = a[o]; h[1][r][c0 + o] = b[o]; h[2][r][c0 + o] = aa[o]; h[3][r][c0 + o] = bb[o];
      h[4][r][c0 + o] = ab[o];
    }
  }
  __syncthreads();
  float sum_l1 = 0.f, sum_s = 0.f, sum_w = 0.f;
  constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;  // pytorch_ssim.py:39-40
  {  // vertical pass + SSIM + partials: VRUN outputs of column c from VRUN + 10 rows
    const int c = tid % TW, r0 = (tid / TW) * VRUN;
    float acc[5][VRUN];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
      for (int o = 0; o < VRUN; ++o) acc[m][o] = 0.f;
#pragma unroll
    for (int k = 0; k < VRUN + LW - 1; ++k) {
      float hv[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) hv[m] = h[m][r0 + k][c];
#pragma unroll
      for (int o = 0; o < VRUN; ++o) {
        const int tp = k - o;
        if (tp >= 0 && tp < LW) {
#pragma unroll
          for (int m = 0; m < 5; ++m) acc[m][o] += win.g[tp] * hv[m];
        }
      }
    }
    const int xx = x0 + c;
#pragma unroll
    for (int o = 0; o < VRUN; ++o) {
      const int r = r0 + o, yy = y0 + r;
      if (yy >= H || xx >= W) continue;
      const float mu1 = acc[0][o], mu2 = acc[1][o], e11 = acc[2][o], e22 = acc[3][o], e12 = acc[4][o];
      const float s11 = e11 - mu1 * mu1, s22 = e22 - mu2 * mu2, s12 = e12 - mu1 * mu2;
      const float A1 = 2.f * mu1 * mu2 + C1, A2 = 2.f * s12 + C2;
      // Where a sum of two products leaves the compiler the choice of which one to fuse, the fused form is written out
      // (fmaf), here and below, so that both instances round alike whatever else is compiled around them (w == 1 gives
      // the bits of egs_gau_loss).
      const float B1 = __builtin_fmaf(mu1, mu1, mu2 * mu2) + C1, B2 = s11 + s22 + C2;
      // two v_rcp_f32 (1 ulp) instead of three IEEE divisions (~10 instructions each): B1, B2 >= C1, C2 > 0
      const float rB1 = __builtin_amdgcn_rcpf(B1), rB2 = __builtin_amdgcn_rcpf(B2);
      const float inv = rB1 * rB2;
      const float A12 = A1 * A2;
      const float S = A12 * inv;  // pytorch_ssim.py:42-43
      // dS/d(mu1, E11, E12) with sigma1_sq = E11 - mu1^2, sigma12 = E12 - mu1 mu2:  dA1 = A2 inv, dA2 = A1 inv,
      // dB1 = -S rB1, dB2 = -S rB2
      const float dA2 = A1 * inv, dB2 = -S * rB2;
      const float dA12 = __builtin_fmaf(A2, inv, -dA2);     // dA1 - dA2
      const float dB12 = __builtin_fmaf(-S, rB1, -dB2);     // dB1 - dB2
      const float pm = __builtin_fmaf(2.f * mu2, dA12, 2.f * mu1 * dB12);
      const float ad = fabsf(sx[r + LR][c + LR] - sy[r + LR][c + LR]);
      const size_t off = plane + (size_t)yy * W + xx;
      if constexpr (WEIGHTED) {   // d(sum of w S)/d(mu1, E11, E12): the gradient body convolves the weighted maps
        const float w = wv[o];
        Pm[off] = w * pm;
        P11[off] = w * dB2;
        P12[off] = w * (2.f * dA2);
        sum_s = __builtin_fmaf(A12, inv * w, sum_s);
        sum_l1 = __builtin_fmaf(w, ad, sum_l1);
        sum_w += w;
      } else {
        Pm[off] = pm;
        P11[off] = dB2;
        P12[off] = 2.f * dA2;
        sum_s = __builtin_fmaf(A12, inv, sum_s);
        sum_l1 += ad;
      }
    }
  }
  sum_l1 = wave_sum(sum_l1); sum_s = wave_sum(sum_s);
  if constexpr (WEIGHTED) sum_w = wave_sum(sum_w);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sum_l1; red[1][tid >> 6] = sum_s;
    if constexpr (WEIGHTED) red[2][tid >> 6] = sum_w;
  }
  __syncthreads();
  if (tid == 0) {  // one pair per TILE (not per workgroup): the summation order does not depend on the grid size
    partials[2 * (size_t)t] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    partials[2 * (size_t)t + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if constexpr (WEIGHTED) {
      if (t < gx * gy) wparts[t] = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    }
  }
  __syncthreads();  // the next tile overwrites sx / sy / red
  }
}

// loss_out = {loss, l1, ssim}; fixed summation order -> bit-reproducible
__device__ __forceinline__ void loss_finalize(int nparts, const float* __restrict__ partials, float lambda,
                                              float inv_count, float* __restrict__ loss_out, double (*red)[4]) {
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) { a += partials[2 * (size_t)i]; b += partials[2 * (size_t)i + 1]; }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double l1 = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) * inv_count;
    const double ss = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) * inv_count;
    loss_out[0] = (float)((1.0 - lambda) * l1 + lambda * (1.0 - ss));  // pytorch_ssim.py:63-66
    loss_out[1] = (float)l1;
    loss_out[2] = (float)ss;
  }
}

// ---- WEIGHTED: what a workgroup derives from sum(w) ----------------------------------------------------------------
// sum(w) from the forward body's channel-0 tile sums, in loss_finalize's order (a thread's strided run in double, the
// wave, the four waves): whoever calls this with the same `wparts` gets the same bits.  `red` (4 doubles) is free again
// on return.
__device__ __forceinline__ double weight_total(int nw, const float* __restrict__ wparts, double* red) {
  double a = 0.0;
  for (int i = threadIdx.x; i < nw; i += 256) a += wparts[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  const double s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}
// 1 / M with M = 3 sum(w), and the two gradient coefficients, formed exactly as egs_gau_loss forms them on the host from
// M = 3 H W (w == 1: the same bits).  sum(w) == 0: all three are 0.
struct WeightedScale { float inv_count, c_l1, c_ssim; };
__device__ __forceinline__ WeightedScale weighted_scale(double sum_w, float lambda, float grad_scale) {
  WeightedScale ws;
  ws.inv_count = sum_w > 0.0 ? (float)(1.0 / (3.0 * sum_w)) : 0.f;
  ws.c_l1 = grad_scale * (1.f - lambda) * ws.inv_count;
  ws.c_ssim = -grad_scale * lambda * ws.inv_count;
  return ws;
}
// loss_out[4] = {loss, l1, ssim, sum(w)}; sum(w) == 0: {0, 0, 1, 0} (one workgroup)
__device__ __forceinline__ void loss_finalize_weighted(int nparts, const float* __restrict__ partials, float lambda,
                                                       float inv_count, double sum_w, float* __restrict__ loss_out,
                                                       double (*red)[4]) {
  loss_finalize(nparts, partials, lambda, inv_count, loss_out, red);
  if (threadIdx.x == 0) {
    loss_out[3] = (float)sum_w;
    if (!(sum_w > 0.0)) { loss_out[0] = 0.f; loss_out[1] = 0.f; loss_out[2] = 1.f; }
  }
}

// loss_out != NULL: workgroup 0 also reduces the forward kernel's per-tile partials to {loss, l1, ssim} (what
// k_loss_finalize does as a launch of its own: 8 us of a training step for a few thousand additions).
// WEIGHTED: c_l1, c_ssim and inv_count are NOT taken from the arguments: every workgroup forms them from `wparts`
// (`nw` tile sums), lambda and grad_scale before its tile loop; the L1 term is c_l1 w sign(x - y); loss_out has 4 entries.
template <bool WEIGHTED>
__device__ __forceinline__ void ssim_bwd_body(int H, int W, int gx, int gy, LossWin win,
                                              const float* __restrict__ img, const float* __restrict__ gt,
                                              const float* __restrict__ Pm, const float* __restrict__ P11,
                                              const float* __restrict__ P12, float c_l1, float c_ssim,
                                              float* __restrict__ dimg, int nparts,
                                              const float* __restrict__ partials, float lambda, float inv_count,
                                              float* __restrict__ loss_out, const float* __restrict__ weight,
                                              const float* __restrict__ wparts, int nw, float grad_scale) {
  __shared__ float s[3][IH][IW + 1];
  __shared__ float h[3][IH][TW + 1];
  __shared__ double fred[2][4];
  const int tid = threadIdx.x;
  const int ntiles = gx * gy * 3;
  float fa[NLOAD], fb[NLOAD], fd[NLOAD];  // halo tile of the three derivative maps in flight (see ssim_fwd_body)
  auto fetch = [&](int t) {
    const TileAt T = tile_at(t, gx, gy, H, W);
#pragma unroll
    for (int j = 0; j < NLOAD; ++j) {
      int r, c; size_t off;
      fa[j] = 0.f; fb[j] = 0.f; fd[j] = 0.f;
      const int i = tid + 256 * j;
      if (i < IH * IW && tile_src(i, T.x0, T.y0, H, W, r, c, off)) {
        fa[j] = Pm[T.plane + off]; fb[j] = P11[T.plane + off]; fd[j] = P12[T.plane + off];
      }
    }
  };
  const TileWalk tw = tile_walk(ntiles);
  int t = tw.t;
  if (t < tw.end) fetch(t);
  if constexpr (WEIGHTED) {
    const double sum_w = weight_total(nw, wparts, fred[0]);
    const WeightedScale sc = weighted_scale(sum_w, lambda, grad_scale);
    c_l1 = sc.c_l1; c_ssim = sc.c_ssim;
    if (blockIdx.x == 0) loss_finalize_weighted(nparts, partials, lambda, sc.inv_count, sum_w, loss_out, fred);
  } else {
    if (loss_out && blockIdx.x == 0) loss_finalize(nparts, partials, lambda, inv_count, loss_out, fred);
  }
  for (; t < tw.end; t += tw.step) {
  const TileAt T = tile_at(t, gx, gy, H, W);
  const int x0 = T.x0, y0 = T.y0;
  const size_t plane = T.plane;
  // this thread's VRUN output pixels: x, y (and w) are only needed at the very end -- fetched first, consumed last
  const int oc = tid % TW, or0 = (tid / TW) * VRUN;
  float px[VRUN], py[VRUN], pw[VRUN];
#pragma unroll
  for (int o = 0; o < VRUN; ++o) {
    const int yy = y0 + or0 + o, xx = x0 + oc;
    px[o] = 0.f; py[o] = 0.f;
    if (yy < H && xx < W) { px[o] = img[plane + (size_t)yy * W + xx]; py[o] = gt[plane + (size_t)yy * W + xx]; }
    if constexpr (WEIGHTED) {
      pw[o] = 0.f;
      if (yy < H && xx < W) pw[o] = weight[(size_t)yy * W + xx];
    }
  }
#pragma unroll
  for (int j = 0; j < NLOAD; ++j) {
    const int i = tid + 256 * j;
    if (i < IH * IW) { const int r = i / IW, c = i - r * IW; s[0][r][c] = fa[j]; s[1][r][c] = fb[j]; s[2][r][c] = fd[j]; }
  }
  __syncthreads();
  if (t + tw.step < tw.end) fetch(t + tw.step);
  if (tid < IH * HSEG) {  // horizontal pass, HRUN outputs per thread (see ssim_fwd_body)
    const int r = tid % IH, c0 = (tid / IH) * HRUN;
    float acc[3][HRUN];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int o = 0; o < HRUN; ++o) acc[m][o] = 0.f;
#pragma unroll
    for (int k = 0; k < HRUN + LW - 1; ++k) {
      float sv[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) sv[m] = s[m][r][c0 + k];
#pragma unroll
      for (int o = 0; o < HRUN; ++o) {
        const int tp = k - o;
        if (tp >= 0 && tp < LW) {
#pragma unroll
          for (int m = 0; m < 3; ++m) acc[m][o] += win.g[tp] * sv[m];
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int o = 0; o < HRUN; ++o) h[m][r][c0 + o] = acc[m][o];
  }
  __syncthreads();
  {  // vertical pass, VRUN outputs per thread
    const int c = oc, r0 = or0;
    float acc[3][VRUN];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int o = 0; o < VRUN; ++o) acc[m][o] = 0.f;
#pragma unroll
    for (int k = 0; k < VRUN + LW - 1; ++k) {
      float hv[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) hv[m] = h[m][r0 + k][c];
#pragma unroll
      for (int o = 0; o < VRUN; ++o) {
        const int tp = k - o;
        if (tp >= 0 && tp < LW) {
#pragma unroll
          for (int m = 0; m < 3; ++m) acc[m][o] += win.g[tp] * hv[m];
        }
      }
    }
    const int xx = x0 + c;
#pragma unroll
    for (int o = 0; o < VRUN; ++o) {
      const int yy = y0 + r0 + o;
      if (yy >= H || xx >= W) continue;
      const size_t off = plane + (size_t)yy * W + xx;
      const float x = px[o], y = py[o];
      const float dS = acc[0][o] + 2.f * x * acc[1][o] + y * acc[2][o];   // d(sum of the SSIM map)/dx
      const float df = x - y;
      float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);  // torch.abs' subgradient: sign(0) = 0
      // (w == 0: +0 whatever x - y is -- what lies outside the weighted region leaves no trace, not even a sign of zero)
      if constexpr (WEIGHTED) sg = pw[o] != 0.f ? pw[o] * sg : 0.f;
      dimg[off] = __builtin_fmaf(c_l1, sg, c_ssim * dS);   // (written out: see ssim_fwd_body)
    }
  }
  __syncthreads();  // the next tile overwrites s / h
  }
}
#endif  // __HIPCC__

}  // namespace egs
