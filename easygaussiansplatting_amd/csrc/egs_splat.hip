// Host orchestration of splat / splatB (reference gsplatcu/gausplat.cu:24-159) and their C-ABI entry points
// (include/egs_hip.h): emission + tile sort + ranges + draw, and the backward draw into packed gradient records.
// The kernels live in egs_sort.hip, egs_bin.hip, egs_draw.hip and egs_segments.hip (interfaces: egs_raster.h).
#include "egs_raster.h"

#include <algorithm>
#include <cstring>

namespace egs {

static int tile_bits(int T) {
  int b = 1;
  while ((1 << b) < T) ++b;
  return b;
}

struct DrawLayout {
  uint32_t *tkeys, *tkeys_alt, *gsid_alt;
  float4* rec;
  int32_t* order;   // dispatch order of the tiles (k_tile_order)
  SortWs sort;
};
static size_t draw_ws_bytes(int n, int64_t P, int width, int height) {
  const size_t N = (size_t)(n > 0 ? n : 1), PP = (size_t)(P > 0 ? P : 1);
  const size_t ord = (size_t)div_up(width, EGS_TILE) * div_up(height, EGS_TILE);   // the tiles' dispatch order
  return 3 * align_up(PP * 4, 256) + align_up(N * 48, 256) + align_up(ord * 4, 256) + sort_ws_bytes(P) + 4096;
}
static bool draw_carve(void* ws, size_t bytes, int n, int64_t P, int width, int height, DrawLayout* L) {
  Carver cv(ws, bytes);
  const size_t N = (size_t)(n > 0 ? n : 1), PP = (size_t)(P > 0 ? P : 1);
  L->tkeys = cv.take<uint32_t>(PP);
  L->tkeys_alt = cv.take<uint32_t>(PP);
  L->gsid_alt = cv.take<uint32_t>(PP);
  L->rec = cv.take<float4>(3 * N);
  L->order = cv.take<int32_t>((size_t)div_up(width, EGS_TILE) * div_up(height, EGS_TILE));
  return sort_ws_carve(cv, P, &L->sort) && cv.ok();
}

// [records | packed gradients | tile dispatch order (bounded: larger images keep the plain tile map)]
constexpr size_t BWD_ORDER_CAP = (size_t)1 << 18;   // tiles: up to 8192 x 8192 pixels

static DrawExtras draw_extras(const EgsExtras* e) {   // (the forward kernel reads the outputs, the backward the dl_*)
  DrawExtras ex = {};
  if (!e) return ex;
  ex.depths = e->depths;
  ex.depth_out = e->depth_out;
  ex.alpha_out = e->alpha_out;
  ex.dl_depth = e->dloss_ddepth;
  ex.dl_alpha = e->dloss_dalpha;
  for (int c = 0; c < 3; ++c) ex.bg[c] = e->background[c];
  return ex;
}

int splat_bwd_packed(int n, int64_t patches, int width, int height, const EgsPolicy* pol, const SplatSource& src,
                     const SplatForward& fwd, const float* dloss_dgammas, void* ws, const SplatCarry& carry,
                     float** gpack_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const float4* rec = src.rec ? (const float4*)src.rec : (const float4*)ws;
  // [N][12] packed gradient records: the caller's (already zeroed by the forward draw kernel) or a piece of ws
  float* gpack = carry.grad_records ? carry.grad_records : (float*)((char*)ws + align_up((size_t)n * 48, 256));
  *gpack_out = gpack;
  if (!carry.grad_records) EGS_HIP(hipMemsetAsync(gpack, 0, (size_t)n * 48, s));
  if (patches == 0) return 0;
  EGS_CHECK_ARG(fwd.contrib && fwd.final_tau && fwd.ranges && fwd.gsid && dloss_dgammas);
  EGS_CHECK_ARG(!carry.extras || (carry.extras->depths && !carry.seg_ws));   // (extras: the unsplit kernels only)
  EGS_CHECK_ARG(!(carry.absgrad && carry.extras));                           // (no ABS + EXTRA instance)
  // (without records they are packed here: from all four tensors, and from the pixel boxes unless the policy is the
  // tile footprint's)
  EGS_CHECK_ARG(src.rec || (src.us && src.cinv2ds && src.alphas && src.colors && (src.areas || pol->footprint == 0)));
  DrawParams dp = make_draw_params(width, height, pol, true);
  dp.masked = (carry.masked_lists && pol->footprint == 0 && pol->alpha_skip > 0.f) ? 1 : 0;
  if (!src.rec) {
    const int rc = pack_records(n, width, height, pol->footprint, pol->alpha_skip, src.us, src.cinv2ds, src.alphas,
                                src.colors, src.areas, (float4*)ws, nullptr, nullptr, nullptr, s);
    if (rc) return rc;
  }
  if (carry.seg_ws) {   // the forward pass split its long lists (egs_splat_draw_rec_seg): one wave per segment
    SegArgs sga;
    const size_t hw = (size_t)width * height;
    const size_t scratch = carry.rebuild ? align_up(20 * hw, 256) + 256 : 0;
    if (pol->footprint != 0 || !(pol->alpha_skip > 0.f) || !(pol->tau_stop > 0.f) || carry.seg_ws_bytes <= scratch ||
        !seg_carve(carry.seg_ws, carry.seg_ws_bytes - scratch, dp.T, &sga)) {
      set_error(EGS_ERR_WORKSPACE, "segment workspace too small (or a policy without a skip / stop threshold)", __FILE__, __LINE__);
      return EGS_ERR_WORKSPACE;
    }
    // (the grid covers the workspace's item capacity -- tiles + state slots, what egs_seg_ws_bytes sized it for -- not a
    // bound formed from the CURRENT egs_seg_config: the render's own L is in the workspace header)
    const int grid = sga.item_cap;
    if (carry.rebuild) {
      sga.rebuild = 1;
      char* sc = (char*)(((uintptr_t)carry.seg_ws + carry.seg_ws_bytes - scratch + 255) & ~(uintptr_t)255);
      float* simg = (float*)sc;
      int32_t* scont = (int32_t*)(sc + 12 * hw);
      float* stau = (float*)(sc + 16 * hw);
      DrawParams fp = make_draw_params(width, height, pol);
      fp.masked = dp.masked;
      int32_t* rg = const_cast<int32_t*>(fwd.ranges);   // (only DIRECT items of an empty tile write it: none here)
      int rc = tile_work_from_contrib(dp, fwd.contrib, nullptr, sga.walk, s);
      if (rc) return rc;
      rc = draw_segments_forward(fp, pol, sga, seg_config(), patches, (const int32_t*)sga.walk, 0, true, nullptr,
                                 carry.seg_hint, false, rg, fwd.gsid, rec, simg, scont, stau, s);
      if (rc) return rc;
    }
    return launch_draw_bwd_seg(dp, pol, fwd.ranges, fwd.gsid, rec, fwd.final_tau, fwd.contrib, dloss_dgammas,
                               gpack, sga, grid, s, carry.absgrad);
  }
  if (carry.tile_order && (carry.keep_forward_order || (size_t)dp.T > BWD_ORDER_CAP)) {
    // the forward pass already dispatched by measured work (that of the camera's previous render, one step or
    // one epoch old -- as good a key for this pass as for that one): no second k_tile_order (8 us); nor for an
    // image whose order does not fit the workspace, which keeps the forward pass's order too
    dp.order = carry.tile_order;
    dp.ngrid = dp.T;
  } else if (carry.tile_order) {
    // the forward draw kernel left behind how far every tile walked its list: order the tiles by THAT (the list
    // length mis-ranks tiles whose pixels saturate early; simulated with the measured work of the 1 M scene:
    // makespan 1.11 x ideal by length, 1.03 x by work)
    int32_t* order = (int32_t*)((char*)ws + 2 * align_up((size_t)n * 48, 256));
    const int32_t* wk = carry.tile_order + dp.T;      // [work | walk] of the forward draw
    const int rc = tile_order_enqueue(dp, order, BWD_ORDER_CAP, fwd.ranges, s, wk,
                                      carry.seg_hint ? wk + dp.T : nullptr, carry.seg_hint);
    if (rc) return rc;
  } else {
    // no record of the forward pass (the seven-op surface: splatB only gets tensors): the work measure is rebuilt
    // from `contrib`, exactly as k_draw would have left it, and the tiles are ordered by it (k_draw_bwd 465 ->
    // 445 us against ordering by list length, for a 4-us kernel)
    int32_t* order = (int32_t*)((char*)ws + 2 * align_up((size_t)n * 48, 256));
    int32_t* work = nullptr;
    int32_t* walk = nullptr;
    if (2 * (size_t)dp.T <= BWD_ORDER_CAP) {
      work = order + dp.T;
      if (carry.seg_hint && 3 * (size_t)dp.T <= BWD_ORDER_CAP) walk = work + dp.T;
      const int rc = tile_work_from_contrib(dp, fwd.contrib, work, walk, s);
      if (rc) return rc;
    }
    const int rc = tile_order_enqueue(dp, order, BWD_ORDER_CAP, fwd.ranges, s, work, walk,
                                      walk ? carry.seg_hint : nullptr);
    if (rc) return rc;
  }
  const DrawExtras ex = draw_extras(carry.extras);
  return launch_draw_bwd(dp, pol, fwd.ranges, fwd.gsid, rec, fwd.final_tau, fwd.contrib, dloss_dgammas, gpack,
                         carry.extras ? &ex : nullptr, s, carry.absgrad);
}
}  // namespace egs

using namespace egs;

extern "C" size_t egs_splat_draw_ws_bytes(int n, int64_t patches, int width, int height) {
  return draw_ws_bytes(n, patches, width, height);
}

// What the records-form draw call adds to the literal op; every field may be 0 / NULL (egs_splat_draw: all of them).
struct DrawOptions {
  const uint32_t* patches_dev;     // != NULL: `patches` is only the capacity of gsid_per_patch / ws_draw, the real
                                   // count is read on the device (the host has not seen it yet)
  int32_t* tile_order;             // (egs_tile_order_len ints) the dispatch order of the tiles is written there, for
                                   // the backward pass to reuse (otherwise it lives in ws_draw and the backward pass
                                   // computes its own)
  float* grad_records;             // ([N][12] floats) zeroed on the side by the draw kernel for the coming backward pass
  const int32_t* prev_tile_work;   // (T ints) the work the draw kernel measured per tile the LAST time this camera was
                                   // rendered -- a much better sort key for the dispatch order than the list length
                                   // (pixels saturate)
  int order_ready;                 // != 0: tile_order already holds a dispatch order (an earlier render through the
                                   // SAME buffer left it there): it is used as it stands, no k_tile_order launch; the
                                   // work part is still rewritten by the draw
  int flags;                       // EGS_DRAW_CULLED_LISTS: the binning stage counted the footprint-culled tiles
                                   // (egs_fused_forward with EGS_FUSED_CULLED_LISTS): the lists are emitted with block
                                   // masks in the high bits of their values and drawn from those; _MASKED_LISTS: the
                                   // same for the reference's lists (egs_splat_bin_pack); _SEG_HISTORY: the walk part
                                   // of tile_order holds what an earlier render of this camera measured; _SEG_SPECULATE
  int32_t* gsid_plain;             // (with EGS_DRAW_MASKED_LISTS) receives the list values without their masks
  void* seg_ws;                    // (egs_seg_ws_bytes) long lists are split over several waves (k_draw_seg; the
  size_t seg_ws_bytes;             // backward pass then takes the same workspace)
  uint32_t* seg_hint;              // (page-locked) receives the longest list of this render
  int32_t* walk_word;              // (with seg_hint) the caller's PERSISTENT device word (one per problem size and
                                   // stream, -1 before its first use) in which this render's draw items gather its
                                   // longest walk; the range kernel of this call first publishes what the previous
                                   // render left there into seg_hint[1]
  const EgsExtras* extras;         // (unsplit lists only) also depth / opacity maps and a background (k_draw_extra)
};

static int splat_draw_impl(int n, int64_t patches, int width, int height, const EgsPolicy* pol, const SplatSource& src,
                           const void* ws_bin, void* ws_draw, size_t ws_draw_bytes, float* image, int32_t* contrib,
                           float* final_tau, int32_t* patch_range_per_tile, int32_t* gsid_per_patch,
                           const DrawOptions& o, void* stream) {
  EGS_CHECK_ARG(n >= 0 && patches >= 0 && patches < (int64_t)0x7FFFFFFF && width > 0 && height > 0 && pol);
  EGS_CHECK_ARG(image && contrib && final_tau && patch_range_per_tile);
  EGS_CHECK_ARG(!o.extras || ((o.extras->depths || n == 0) && !o.seg_ws));
  hipStream_t s = (hipStream_t)stream;
  DrawParams dp = make_draw_params(width, height, pol);
  const bool masked = (o.flags & (EGS_DRAW_CULLED_LISTS | EGS_DRAW_MASKED_LISTS)) && pol->footprint == 0 &&
                      pol->alpha_skip > 0.f;
  EGS_CHECK_ARG(!masked || n < (1 << EGS_GSID_BITS));
  dp.masked = masked ? 1 : 0;
  if (o.grad_records && n > 0 && (patches == 0)) EGS_HIP(hipMemsetAsync(o.grad_records, 0, (size_t)n * 48, s));
  if (n == 0 || patches == 0) {  // nothing to draw: all outputs are zero
    const size_t hw = (size_t)width * height;
    EGS_HIP(hipMemsetAsync(patch_range_per_tile, 0, (size_t)dp.T * 8, s));
    EGS_HIP(hipMemsetAsync(image, 0, 12 * hw, s));
    EGS_HIP(hipMemsetAsync(contrib, 0, 4 * hw, s));
    EGS_HIP(hipMemsetAsync(final_tau, 0, 4 * hw, s));
    if (o.extras) {   // T = 1 everywhere: the background, no depth, no opacity
      for (int c = 0; c < 3; ++c) {
        uint32_t bits;
        memcpy(&bits, &o.extras->background[c], 4);
        EGS_HIP(hipMemsetD32Async((hipDeviceptr_t)(image + c * hw), (int)bits, hw, s));
      }
      if (o.extras->depth_out) EGS_HIP(hipMemsetAsync(o.extras->depth_out, 0, 4 * hw, s));
      if (o.extras->alpha_out) EGS_HIP(hipMemsetAsync(o.extras->alpha_out, 0, 4 * hw, s));
    }
    if (o.tile_order) {
      // the caller keeps [order | work] between renders and will trust it next time (order_ready): it must hold
      // a valid permutation and the work of THIS render (none) whatever happened here
      if (!o.order_ready) {
        const int rc = tile_order_enqueue(dp, o.tile_order, (size_t)dp.T, patch_range_per_tile, s, nullptr);
        if (rc) return rc;
      }
      EGS_HIP(hipMemsetAsync(o.tile_order + dp.T, 0, (size_t)dp.T * 8, s));   // work and walk
    }
    if (o.seg_ws) {   // a backward pass may still be handed the workspace: no items, nothing split
      SegArgs sa;
      if (seg_carve(o.seg_ws, o.seg_ws_bytes, dp.T, &sa)) EGS_HIP(hipMemsetAsync(sa.hdr, 0, SEG_HDR * 4, s));
    }
    return 0;
  }
  EGS_CHECK_ARG(ws_bin && ws_draw && gsid_per_patch);
  EGS_CHECK_ARG(src.rec || (src.us && src.cinv2ds && src.alphas && src.colors && src.areas));
  BinLayout B;
  if (!bin_carve(const_cast<void*>(ws_bin), bin_ws_bytes(n), n, &B)) return EGS_ERR_WORKSPACE;
  DrawLayout D;
  if (!draw_carve(ws_draw, ws_draw_bytes, n, patches, width, height, &D)) {
    set_error(EGS_ERR_WORKSPACE, "draw workspace too small", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  const int tb = tile_bits(dp.T);
  const int passes = sort_passes(0, tb);
  uint32_t* gs_primary = (uint32_t*)gsid_per_patch;
  // choose the emission buffers so that the sorted result lands in the primary ones
  uint32_t* k0 = (passes & 1) ? D.tkeys_alt : D.tkeys;
  uint32_t* k1 = (passes & 1) ? D.tkeys : D.tkeys_alt;
  uint32_t* v0 = (passes & 1) ? D.gsid_alt : gs_primary;
  uint32_t* v1 = (passes & 1) ? gs_primary : D.gsid_alt;
  int rc = bin_emit(n, dp.gx, B, k0, v0, (uint32_t)patches, patch_range_per_tile, 2 * dp.T, dp.masked, D.sort.sup,
                    (uint32_t)D.sort.sup_words, s);
  if (rc) return rc;
  const float4* rec = src.rec ? (const float4*)src.rec : D.rec;
  if (!src.rec) {
    rc = pack_records(n, width, height, pol->footprint, pol->alpha_skip, src.us, src.cinv2ds, src.alphas, src.colors,
                      src.areas, D.rec, nullptr, nullptr, nullptr, s);
    if (rc) return rc;
  }
  rc = radix_sort(patches, k0, v0, k1, v1, 0, tb, D.sort, s, nullptr, o.patches_dev);
  if (rc) return rc;
  SegArgs sga;
  const bool seg = o.seg_ws && pol->footprint == 0 && pol->alpha_skip > 0.f && pol->tau_stop > 0.f &&
                   dp.T <= (int)SEG_TILE_MASK && seg_carve(o.seg_ws, o.seg_ws_bytes, dp.T, &sga);
  // (the range kernel clears the bins and counters of the segment plan on the side, and publishes the longest walk of the
  // previous render on this stream)
  rc = tile_ranges(patches, D.tkeys, patch_range_per_tile, o.patches_dev,
                   (const uint32_t*)(o.gsid_plain ? gsid_per_patch : nullptr), o.gsid_plain, s, seg ? sga.hdr : nullptr,
                   seg ? SEG_PLAN_WORDS : 0, o.walk_word, o.seg_hint);
  if (rc) return rc;
  if (o.seg_ws && !seg) {
    set_error(EGS_ERR_WORKSPACE, "segment workspace too small (or a policy without a skip / stop threshold)", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  if (seg) {
    const SegConfig cfg = seg_config();   // (read once per render: the plan kernel leaves L in the workspace header)
    const int32_t* hist = (o.tile_order && (o.flags & EGS_DRAW_SEG_HISTORY)) ? o.tile_order + 2 * dp.T : nullptr;
    sga.hist_walk = o.tile_order ? o.tile_order + 2 * dp.T : nullptr;
    const int speculate = (o.flags & EGS_DRAW_SEG_SPECULATE) ? 1 : 0;    // (with a walk on record: where that looks stale)
    if (o.tile_order) dp.work_out = o.tile_order + dp.T;
    if (o.grad_records) {   // (zero_per: set by draw_segments_forward from its grid)
      dp.zero_buf = (float4*)o.grad_records;
      dp.zero_n4 = (uint32_t)(3 * (size_t)n);
    }
    return draw_segments_forward(dp, pol, sga, cfg, patches, hist, speculate, hist || speculate, o.walk_word,
                                 o.seg_hint, true, patch_range_per_tile, gsid_per_patch, rec, image, contrib, final_tau, s);
  }
  if (o.order_ready && o.tile_order && dp.T <= TILE_ORDER_MAX_T) {
    dp.order = o.tile_order;
    dp.ngrid = dp.T;
  } else {
    // (prev_tile_work is the work part of a camera's own buffer: its walk part lies T ints behind it)
    // (no hint words from here, as in round 5 -- the walk of the camera's PREVIOUS render is stale after reset_alpha and
    // would overwrite what the range kernel just published; the draw waves gather both words of this render)
    rc = tile_order_enqueue(dp, o.tile_order ? o.tile_order : D.order, (size_t)dp.T, patch_range_per_tile, s,
                            o.prev_tile_work, nullptr, o.walk_word ? nullptr : o.seg_hint);
    if (rc) return rc;
  }
  if (o.tile_order) { dp.work_out = o.tile_order + dp.T; dp.walk_out = dp.work_out + dp.T; }
  if (o.tile_order) dp.walk_max = o.walk_word;     // (every render refreshes the host's hint, one render late)
  if (o.grad_records) {
    dp.zero_buf = (float4*)o.grad_records;
    dp.zero_n4 = (uint32_t)(3 * (size_t)n);
    dp.zero_per = (dp.zero_n4 + (uint32_t)draw_grid(dp) - 1) / (uint32_t)draw_grid(dp);
  }
  const DrawExtras ex = draw_extras(o.extras);
  return launch_draw(dp, pol, patch_range_per_tile, gsid_per_patch, rec, image, contrib, final_tau,
                     o.extras ? &ex : nullptr, s);
}

// the literal op: the records are packed here from the tensors, `patches` is the count the host read back
extern "C" int egs_splat_draw(int n, int64_t patches, int width, int height, const float* us,
                              const float* cinv2ds, const float* alphas, const float* colors,
                              const int32_t* areas, const EgsPolicy* pol, const void* ws_bin, void* ws_draw,
                              size_t ws_draw_bytes, float* image, int32_t* contrib, float* final_tau,
                              int32_t* patch_range_per_tile, int32_t* gsid_per_patch, void* stream) {
  return splat_draw_impl(n, patches, width, height, pol,
                         {.us = us, .cinv2ds = cinv2ds, .alphas = alphas, .colors = colors, .areas = areas}, ws_bin,
                         ws_draw, ws_draw_bytes, image, contrib, final_tau, patch_range_per_tile, gsid_per_patch,
                         DrawOptions{}, stream);
}

// the draw stage from the packed records, with everything a host may add (include/egs_hip.h)
extern "C" int egs_splat_draw_rec_seg(int n, int64_t patches, const uint32_t* total_patches, int width, int height,
                                      const void* rec, const EgsPolicy* pol, const void* ws_bin, void* ws_draw,
                                      size_t ws_draw_bytes, float* image, int32_t* contrib, float* final_tau,
                                      int32_t* patch_range_per_tile, int32_t* gsid_per_patch, int32_t* tile_order,
                                      float* grad_records, const int32_t* prev_tile_work, int order_ready, int flags,
                                      void* seg_ws, size_t seg_ws_bytes, uint32_t* seg_hint, int32_t* walk_word,
                                      int32_t* gsid_plain, void* stream, const EgsExtras* extras) {
  EGS_CHECK_ARG((rec || n == 0) && (!total_patches || patches > 0));
  EGS_CHECK_ARG(!gsid_plain || ((((uintptr_t)gsid_plain | (uintptr_t)gsid_per_patch) & 15) == 0));
  return splat_draw_impl(n, patches, width, height, pol, {.rec = rec}, ws_bin, ws_draw, ws_draw_bytes, image, contrib,
                         final_tau, patch_range_per_tile, gsid_per_patch,
                         {.patches_dev = total_patches, .tile_order = tile_order, .grad_records = grad_records,
                          .prev_tile_work = prev_tile_work, .order_ready = order_ready, .flags = flags,
                          .gsid_plain = gsid_plain, .seg_ws = seg_ws, .seg_ws_bytes = seg_ws_bytes, .seg_hint = seg_hint,
                          .walk_word = walk_word, .extras = extras},
                         stream);
}

extern "C" size_t egs_splat_bwd_ws_bytes(int n) {
  return 2 * align_up((size_t)(n > 0 ? n : 1) * 48, 256) + BWD_ORDER_CAP * 4 + 256;
}
extern "C" size_t egs_seg_rebuild_ws_bytes(int64_t patch_capacity, int width, int height) {
  return egs_seg_ws_bytes(patch_capacity, width, height) + align_up((size_t)20 * width * height, 256) + 512;
}

// what the two splatB entry points share: the argument checks, n == 0, the workspace size, the draw pass into the
// packed gradient records and their unpacking into the four outputs
static int splat_bwd_unpacked(int n, int64_t patches, int width, int height, const EgsPolicy* pol,
                              const SplatSource& src, const SplatForward& fwd, const float* dloss_dgammas, void* ws,
                              size_t ws_bytes, const SplatCarry& carry, float* dloss_dus, float* dloss_dcinv2ds,
                              float* dloss_dalphas, float* dloss_dcolors, void* stream) {
  EGS_CHECK_ARG(n >= 0 && patches >= 0 && width > 0 && height > 0 && pol);
  if (n == 0) return 0;
  EGS_CHECK_ARG(ws && dloss_dus && dloss_dcinv2ds && dloss_dalphas && dloss_dcolors);
  if (ws_bytes < egs_splat_bwd_ws_bytes(n)) {
    set_error(EGS_ERR_WORKSPACE, "splat_bwd workspace too small", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  float* gpack = nullptr;
  const int rc = splat_bwd_packed(n, patches, width, height, pol, src, fwd, dloss_dgammas, ws, carry, &gpack, stream);
  if (rc) return rc;
  return unpack_grads(n, gpack, dloss_dus, dloss_dcinv2ds, dloss_dalphas, dloss_dcolors, (hipStream_t)stream);
}

// splatB with everything optional that a host may or may not have kept of its forward pass (include/egs_hip.h)
extern "C" int egs_splat_bwd_seg(int n, int64_t patches, int width, int height, const float* us, const float* cinv2ds,
                                 const float* alphas, const float* colors, const void* rec, const EgsPolicy* pol,
                                 const int32_t* contrib, const float* final_tau, const int32_t* patch_range_per_tile,
                                 const int32_t* gsid_per_patch, const float* dloss_dgammas, void* ws, size_t ws_bytes,
                                 const int32_t* tile_order, float* grad_records, float* dloss_dus,
                                 float* dloss_dcinv2ds, float* dloss_dalphas, float* dloss_dcolors, int flags,
                                 void* seg_ws, size_t seg_ws_bytes, int rebuild, uint32_t* seg_hint, void* stream) {
  // (no `areas` here: without records only the tile-footprint policies can pack; refused before the workspace is sized)
  EGS_CHECK_ARG(n <= 0 || !pol || rec || (us && cinv2ds && alphas && colors && pol->footprint != 1));
  return splat_bwd_unpacked(n, patches, width, height, pol,
                            {.rec = rec, .us = us, .cinv2ds = cinv2ds, .alphas = alphas, .colors = colors},
                            {.contrib = contrib, .final_tau = final_tau, .ranges = patch_range_per_tile,
                             .gsid = gsid_per_patch},
                            dloss_dgammas, ws, ws_bytes,
                            {.tile_order = tile_order, .grad_records = grad_records,
                             .masked_lists = (flags & (EGS_DRAW_CULLED_LISTS | EGS_DRAW_MASKED_LISTS)) != 0,
                             .seg_ws = seg_ws, .seg_ws_bytes = seg_ws_bytes, .rebuild = rebuild, .seg_hint = seg_hint},
                            dloss_dus, dloss_dcinv2ds, dloss_dalphas, dloss_dcolors, stream);
}

// the literal op: tensors only, nothing carried over from the forward pass
extern "C" int egs_splat_bwd(int n, int64_t patches, int width, int height, const float* us,
                             const float* cinv2ds, const float* alphas, const float* colors,
                             const int32_t* areas, const EgsPolicy* pol, const int32_t* contrib,
                             const float* final_tau, const int32_t* patch_range_per_tile,
                             const int32_t* gsid_per_patch, const float* dloss_dgammas, void* ws, size_t ws_bytes,
                             float* dloss_dus, float* dloss_dcinv2ds, float* dloss_dalphas, float* dloss_dcolors,
                             void* stream) {
  return splat_bwd_unpacked(n, patches, width, height, pol,
                            {.us = us, .cinv2ds = cinv2ds, .alphas = alphas, .colors = colors, .areas = areas},
                            {.contrib = contrib, .final_tau = final_tau, .ranges = patch_range_per_tile,
                             .gsid = gsid_per_patch},
                            dloss_dgammas, ws, ws_bytes, SplatCarry{}, dloss_dus, dloss_dcinv2ds, dloss_dalphas,
                            dloss_dcolors, stream);
}
