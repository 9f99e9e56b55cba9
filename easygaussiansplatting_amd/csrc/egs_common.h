// Shared host/device helpers of libegs_hip.so (gfx950 / CDNA4 only: wave64).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>

#include "../../include/egs_hip.h"

#define EGS_MIN_DEPTH 0.2f   // reference kernel.cu:10
#define EGS_BAD_MARKER (-1.f) // reference kernel.cu:11
#define EGS_TILE 16          // reference common.cuh:12 (BLOCK)
#define EGS_WAVE 64

namespace egs {

// ---- error reporting --------------------------------------------------------
void set_error(int code, const char* what, const char* file, int line);

#define EGS_CHECK_ARG(cond)                                                      \
  do {                                                                           \
    if (!(cond)) {                                                               \
      ::egs::set_error(EGS_ERR_BAD_ARG, "bad argument: " #cond, __FILE__, __LINE__); \
      return EGS_ERR_BAD_ARG;                                                    \
    }                                                                            \
  } while (0)

#define EGS_HIP(expr)                                                            \
  do {                                                                           \
    hipError_t e__ = (expr);                                                     \
    if (e__ != hipSuccess) {                                                     \
      ::egs::set_error((int)e__, hipGetErrorString(e__), __FILE__, __LINE__);    \
      return (int)e__;                                                           \
    }                                                                            \
  } while (0)

// after a <<<>>> launch: catches launch-configuration errors without syncing
#define EGS_LAUNCH_OK() EGS_HIP(hipGetLastError())

// ---- optional per-kernel timing (egs_prof_* in the C ABI) -------------------
bool prof_on(const char* name);
void prof_begin(const char* name, hipStream_t s);
void prof_end(hipStream_t s);
struct ProfScope {
  hipStream_t s;
  bool on;
  ProfScope(const char* name, hipStream_t st) : s(st), on(prof_on(name)) {
    if (on) prof_begin(name, s);
  }
  ~ProfScope() {
    if (on) prof_end(s);
  }
};
// launch `kern` on `stream`, bracketed by events when profiling is enabled
#define EGS_LAUNCH(name, kern, grid, block, stream, ...)                 \
  do {                                                                   \
    ::egs::ProfScope ps__(name, stream);                                 \
    hipLaunchKernelGGL(kern, grid, block, 0, stream, __VA_ARGS__);       \
  } while (0)

// ---- runtime flags -> template arguments --------------------------------------
// A kernel's flavour is a set of template arguments; a launch site turns its runtime flags into them once:
//   decltype(&k<false, false>) kern = nullptr;
//   with_bools([&](auto raw, auto aa) { kern = k<raw.value, aa.value>; }, is_raw, is_aa);
//   EGS_LAUNCH(label, kern, grid, block, stream, arguments...);
// calls the generic lambda with one std::true_type / std::false_type per flag (2^flags instantiations of its body:
// exactly the kernel instances it names).  The lambda only picks the instance -- every instance of a template has one
// signature -- so the launch, its arguments and its profiler bracket exist once per site, not once per instance.
template <typename F>
inline void with_bools(F&& f) { f(); }
template <typename F, typename... B>
inline void with_bools(F&& f, bool b0, B... rest) {
  if (b0) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// SH row width (3 (degree + 1)^2 floats; checked by the caller) -> f(std::integral_constant<int, NC>): NC coefficients
// per colour channel
template <typename F>
inline void with_sh_dim(int sh_dim, F&& f) {
  switch (sh_dim) {
    case 3: f(std::integral_constant<int, 1>{}); break;
    case 12: f(std::integral_constant<int, 4>{}); break;
    case 27: f(std::integral_constant<int, 9>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
  }
}

static inline int div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// bump allocator over a caller-supplied workspace (256-B aligned pieces)
struct Carver {
  char* base;
  size_t off;
  size_t cap;
  Carver(void* p, size_t bytes) : base((char*)p), off(0), cap(bytes) {}
  template <typename T>
  T* take(size_t count) {
    size_t start = align_up(off, 256);
    off = start + count * sizeof(T);
    return (T*)(base + start);
  }
  bool ok() const { return off <= cap; }
};

// ---- binning pieces shared by egs_bin.hip (egs_splat_bin) and egs_preprocess.hip (the fused forward
// kernel does getRects + the depth key itself) ---------------------------------------------------------
struct BinParams {
  int W, H, gx, gy;
  int footprint, far_cull, depth_key, mutate;
  int cull_lists;   // lists may drop the tiles of a rect that the footprint alpha' >= alpha_skip cannot reach (fused path)
};
// What the binning stage keeps of a Gaussian (32 bytes, gathered ONCE into depth order by the depth sort's last
// scatter pass): its footprint -- centre u, the conic in "power form" and the threshold m:
//     the Gaussian blends into a pixel  <=>  A dx^2 + 2 Bh dx dy + C dy^2 <= m        (d = pixel - u)
// (A, 2 Bh, C) = -(qxx, qxy, qyy) of the draw record, m = -thr = log2(alpha / alpha_skip): exactly the skip test of
// the draw kernels (kernel.cu:246) -- and its tile rect (getRects, kernel.cu:82-122).  m = +inf: no footprint
// culling, the Gaussian is emitted for every tile of its rect (the reference's lists).
struct BinRec {
  float ux, uy, A, Bh;
  float C, m;
  uint32_t xy;   // x0 | y0 << 16   (tiles)
  uint32_t wh;   // w | h << 16
};
static_assert(sizeof(BinRec) == 32, "BinRec is two dwordx4");
// The compact form the binning stage works with (16 bytes, gathered ONCE into depth order by the depth sort's last
// scatter pass):  {x0 | y0 << 16,  w | h << 16 | flags,  b_lo, b_hi}  (tiles).
//   rect of at most 4 x 4 tiles:  b = 64-bit bitmap of the 8x8 pixel blocks of the rect the footprint reaches, bit
//     8 by + bx relative to the rect's first block (ALL blocks of the rect when the Gaussian is not cullable).  The
//     Gaussian is emitted for the tiles with a block set, the list value's mask is the tile's four bits: emission is
//     bit arithmetic, the square roots of the footprint are taken once per Gaussian, in k_preprocess_fwd.
//   rect of at most 8 x 8 tiles (EGS_CR_TILEMAP, cullable Gaussians only):  b = 64-bit bitmap of the TILES of the rect
//     the footprint reaches, bit 8 ty + tx; emission finds slot r's tile by bit arithmetic and evaluates the two
//     8-row slabs of THAT tile with the full footprint record br[gaussian] for its block mask (11 % of the patches of
//     a ring view of the 1 M scene sit in rects larger than 4 x 4 tiles, 0.3 % of view 0's).
//   larger rect (EGS_CR_BIG):  b_lo = patch count, b_hi != 0: cullable -- k_bin_emit walks the rows of the rect with
//     br[gaussian]; b_hi == 0: every tile of the rect.
//   EGS_CR_ALLTILES (seven-op surface, k_pack_bin): the lists are the REFERENCE's -- every tile of the rect, row-major --
//     and the footprint only supplies the block mask of each tile (possibly empty: the entry stays in the list and is
//     never evaluated).  Rect of at most 4 x 4 tiles: b = the block bitmap as above; EGS_CR_BIG with b_hi == 2: every
//     tile of the rect, masks from br[gaussian].
#define EGS_CR_BIG 0x80000000u
#define EGS_CR_TILEMAP 0x40000000u
#define EGS_CR_ALLTILES 0x20000000u
#define EGS_CR_WH_MASK 0x1FFFFFFFu
struct BinCountOut {  // where k_bin_count's results live inside the bin workspace
  uint4* cr;                       // compact bin record per Gaussian
  BinRec* br;                      // footprint record, written for the cullable Gaussians with a rect larger than 4 x 4 tiles only
  uint32_t *dkeys, *ids, *maxkey;  // maxkey[1 + workgroup] = per-workgroup maximum of the depth keys
  uint32_t* sort_sup;              // the depth sort's superblock sums: the producing kernel ZEROES them on the side
  uint32_t sort_sup_words;
};
// list values of the culled lists (fused path): Gaussian index in the low 28 bits, in the high 4 the 8x8 pixel blocks
// of the tile the footprint reaches (bit k = block (k&1, k>>1)) -- computed ONCE per (tile, Gaussian) at emission
// instead of per entry and draw kernel, and exact where the draw kernels' own box test is conservative
#define EGS_GSID_BITS 28
#define EGS_GSID_MASK 0x0FFFFFFFu
BinParams make_bin_params(int width, int height, const EgsPolicy* pol, bool cull_lists = false);
bool bin_count_outputs(void* ws_bin, size_t ws_bin_bytes, int n, BinCountOut* out);
// everything of egs_splat_bin after k_bin_count (max reduce, depth sort, offsets scan)
// host_totals (nullable): page-locked host uint32[2] the kernels ALSO write {P, max depth key} into (mailbox slot)
int splat_bin_after_count(int n, int key_bits_hint, void* ws_bin, size_t ws_bin_bytes, uint32_t* total_patches,
                          void* stream, uint32_t* host_totals);

// ---- the arguments of the splat stage (egs_splat.hip), grouped by what travels together ----------------------------
// The 2D Gaussians of a draw / backward draw: the packed 48-B records, or the tensors they are packed from.
struct SplatSource {
  const void* rec;       // [N][12] packed records (egs_pack_records / egs_fused_forward); NULL: packed from the tensors
  const float *us, *cinv2ds, *alphas, *colors;   // the op surface's tensors (needed when rec == NULL)
  const int32_t* areas;  // pixel boxes: the pixel-box policy packs from them (always, for the literal egs_splat_draw)
};
// What the forward draw wrote and the backward draw reads (required whenever there are patches).
struct SplatForward {
  const int32_t* contrib;
  const float* final_tau;
  const int32_t* ranges;   // patch_range_per_tile [T][2]
  const int32_t* gsid;     // gsid_per_patch [P]; with masked_lists: the list WITH block masks the forward draw walked
};
// What a host may have carried over from the forward pass to splat_bwd_packed; every field may be 0 / NULL.
struct SplatCarry {
  const int32_t* tile_order;   // the [order | work | walk] buffer the forward draw left: no pass over `contrib`
  float* grad_records;         // [N][12] records ALREADY ZEROED (by the forward draw kernel); NULL: a piece of ws
  bool keep_forward_order;     // dispatch the tiles exactly as tile_order says (EGS_BWD_KEEP_FORWARD_ORDER)
  bool masked_lists;           // gsid carries block masks (culled lists of the fused path, EGS_DRAW_MASKED_LISTS)
  void* seg_ws;                // the segment workspace the forward draw filled (egs_splat_draw_rec_seg), or, with
  size_t seg_ws_bytes;         // rebuild, a fresh one of egs_seg_rebuild_ws_bytes
  int rebuild;                 // != 0: no forward pass left its segment states in seg_ws -- the public splatB is handed
                               // tensors only -- so they are REBUILT first: every tile's walk from `contrib`, then the
                               // forward segment launches over [0, walk) with their pixels going to scratch
  uint32_t* seg_hint;          // page-locked words that learn the longest walk (both paths report it: a host decides
                               // the path of its NEXT call from it)
  const EgsExtras* extras;     // render extras: the EXTRA draw kernel (unsplit lists only)
  bool absgrad;                // the ABS draw kernels: sum |dL/du| per pixel into gpack[i][10..11]
};
// splatB's draw pass into the packed [N][12] gradient records (egs_splat.hip); *gpack is carry.grad_records or points
// into `ws` (egs_splat_bwd_ws_bytes(n), checked by the caller).  Shared by egs_splat_bwd / _seg (+unpack) and
// egs_fused_backward.
int splat_bwd_packed(int n, int64_t patches, int width, int height, const EgsPolicy* pol, const SplatSource& src,
                     const SplatForward& fwd, const float* dloss_dgammas, void* ws, const SplatCarry& carry,
                     float** gpack, void* stream);

// ---- device helpers ---------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// inclusive scan across the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// exclusive scan over a 256-thread block; `total` receives the block sum.
// `smem` must hold >= 4 uint32 and is reused on return after a barrier.
__device__ __forceinline__ uint32_t block256_exclusive_scan(uint32_t v, uint32_t* smem, uint32_t* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t inc = wave_inclusive_scan(v);
  if (lane == 63) smem[wave] = inc;
  __syncthreads();
  uint32_t s0 = smem[0], s1 = smem[1], s2 = smem[2], s3 = smem[3];
  uint32_t off = (wave > 0 ? s0 : 0u) + (wave > 1 ? s1 : 0u) + (wave > 2 ? s2 : 0u);
  if (total) *total = s0 + s1 + s2 + s3;
  __syncthreads();
  return off + inc - v;
}

// sum over the 64 lanes of a wave; result valid in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
#endif

}  // namespace egs
