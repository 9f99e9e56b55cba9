"""Inputs and truth of the binning-chain tests (tests/test_gpu_bin_lists.py, checked without a GPU by
tests/test_bin_cases_cpu.py): hand-built 2D Gaussians whose tile rect and depth key are DICTATED, and the per-tile lists
they must produce, written down by definition.  NumPy only.

A case is a list of Gaussians, each given as the tile rect (x0, y0, w, h) it is meant to cover, the depth key it is meant
to get and a ``form``: FORM_PATCH (it has patches) or one of four ways of having none.  ``build`` derives the three input
arrays of the binning stage from that:

  gsplatcu (rule of bin_count_one / O.get_rects, kernel.cu:105-110): u = 16 x0 + 8 w, radius = 8 w - 8 gives
      trunc((u - r) / 16) = trunc(x0 + 1/2) = x0 and trunc((u + r + 15) / 16) = trunc(x0 + w + 7/16) = x0 + w; the depth
      is the float32 whose product with 1000.f truncates to the key (searched with nextafter from (key + 1/2) / 1000:
      the depth is adjusted, never the expectation).  A depth >= 0.2 has a key >= 200.
        FORM_NEAR   depth 0.1: below MIN_DEPTH, nothing is touched (kernel.cu:97)
        FORM_OFF    u = (-100 - i % 50, 40), radius 5: both x bounds clamp to 0 -- culled in place (kernel.cu:114-119)
        FORM_EMPTY  u = (16 x0, 16 y0 + 8), radius 0: trunc(x0) = trunc(x0 + 15/16), an empty rect ON the screen -- culled
        FORM_REV    radius (-24, 0): x bounds (x0 + 2, x0 - 1), a REVERSED rect.  The reference's unsigned product wraps to
                    ~2^32 patches there; this project defines it as empty (bin_count_one, and O.get_rects since these
                    tests) -- culled
  forward_cpu (pixel box, gausplat.py:204-218): u = 16 x0 + 8 w, radius = 8 w - 1: the box [16 x0 + 1, 16 (x0 + w) - 1]
      (clamped to the image) touches exactly those tiles; the key is the depth's float32 bit pattern.  Nothing is culled
      in place.  FORM_NEAR depth 0.1, FORM_REV depth 150 (beyond 100), FORM_OFF u = -1.5 (W, H), FORM_EMPTY a box clamped
      to nothing at (-50, -50).

A Gaussian without patches has key 0 in the kernels, so in DEPTH order -- the order the scan kernels and k_bin_emit
see -- they form a prefix unless the Gaussians with patches have key 0 too.  Under gsplatcu only a NaN depth does that
(``(uint32_t)NaN == 0``; ``NaN < 0.2`` is false, so it keeps its patches: kernel.cu:61, :97).  The ``counts`` set therefore
comes twice: ``mm`` (keys >= 200: the pattern sits where k_bin_count / k_pack_bin see it, the depth sort moves the
patch-less ones to the front) and ``nan`` (every depth NaN: depth order == index order, the pattern sits where
k_bin_scan_* and k_bin_emit see it).

``reference_lists`` is the definition, not an algorithm: for every tile, the Gaussians whose rect contains it, in
(key, index) order.  No (tile, key, id) triples are sorted."""
import numpy as np

F = np.float32
TILE = 16
WG = 256                       # workgroup of k_bin_count / k_pack_bin / k_bin_emit
SC_TILE = 2048                 # items per workgroup of k_bin_scan_*, and the sort's short tile
RANGE_WG, QUAD = 1024, 4       # k_tile_ranges: keys per workgroup, keys per thread
RS_SHORT = 5 << 19             # the last count on the 8-items-per-thread sort instances
MIN_KEY = 200                  # key of the smallest depth that is not below MIN_DEPTH
SAT = 0xFFFFFFFF
FORM_PATCH, FORM_NEAR, FORM_OFF, FORM_EMPTY, FORM_REV = 0, 1, 2, 3, 4
FORM_NAMES = ("patch", "near", "off", "empty", "rev")


def grid(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def tile_key_bits(T):
    """width of the tile key: tile_bits of egs_splat.hip"""
    b = 1
    while (1 << b) < T:
        b += 1
    return b


def sort_passes(bits):
    return (bits + 7) // 8


def pass_widths(bits):
    """digit widths of the passes: the bits are split evenly (radix_sort)"""
    p = sort_passes(bits)
    w = (bits + p - 1) // p
    return [min(w, bits - s) for s in range(0, bits, w)]


def bit_length(v):
    return int(v).bit_length()


def real_depth_passes(maxkey, hint=32):
    """passes of the depth sort that are no identity pass: the first always runs, a later one iff a key has a bit at or
    above its shift"""
    end = 32 if hint <= 0 or hint > 32 else hint
    ws = pass_widths(end)
    shifts = np.cumsum([0] + ws[:-1])
    return 1 + sum(1 for s in shifts[1:] if (int(maxkey) >> int(s)) != 0)


def depth_for_key(key):
    """float32 depths d with trunc(float32(d * 1000.f)) == key.  Every key in [MIN_KEY, 2^22] has one; above 2^23 the
    product of neighbouring float32 depths with 1000 steps by about 2 and some keys do not exist (2^24 - 1 and 2^24 do):
    asking for one of those fails here, no expectation is bent to fit"""
    k = np.asarray(key, np.float64)
    d = ((k + 0.5) / 1000.0).astype(F)
    for _ in range(32):
        got = np.trunc((d * F(1000)).astype(np.float64))
        lo, hi = got < k, got > k
        if not (lo.any() or hi.any()):
            return d
        d = np.where(lo, np.nextafter(d, F(np.inf)), np.where(hi, np.nextafter(d, F(-np.inf)), d)).astype(F)
    raise AssertionError("no float32 depth for keys %r" % (np.asarray(key)[lo | hi][:8],))


class Case:
    """name, cset, policy ('gsplatcu' | 'forward_cpu'), W, H; per Gaussian: rect [n, 4] = (x0, y0, w, h), key [n] uint32,
    form [n]; depth [n] float32 or None: explicit depths (NaN bit patterns included) where ``given`` is set;
    what: what the case is supposed to contain; claims: name -> value; props: tuples checked by the CPU test"""

    def __init__(self, name, cset, policy, W, H, rect, key, form, what, claims=None, props=(), depth=None, given=None):
        self.name, self.cset, self.policy, self.W, self.H, self.what = name, cset, policy, W, H, what
        self.rect = np.ascontiguousarray(rect, np.int64).reshape(-1, 4)
        self.n = self.rect.shape[0]
        self.key = np.ascontiguousarray(key, np.uint32).reshape(self.n)
        self.form = np.ascontiguousarray(form, np.int64).reshape(self.n)
        self.claims, self.props = dict(claims or {}), list(props)
        self.depth = None if depth is None else np.ascontiguousarray(depth, F)
        self.given = np.zeros(self.n, bool) if given is None else np.asarray(given, bool)
        self._built = None
        self._ref = None

    def __repr__(self):
        return "%s/%s [%s, %d x %d, n = %d]: %s" % (self.cset, self.name, self.policy, self.W, self.H, self.n, self.what)

    def prefix(self, m):
        """the first m Gaussians as a case of their own (no claims)"""
        s = slice(0, m)
        return Case(self.name + "_prefix%d" % m, self.cset, self.policy, self.W, self.H, self.rect[s], self.key[s],
                    self.form[s], self.what + " (first %d)" % m, depth=None if self.depth is None else self.depth[s],
                    given=self.given[s])


def build(case):
    """-> (us [n, 2] float32, areas [n, 2] int32, depths [n] float32): fresh copies"""
    if case._built is None:
        n, i = case.n, np.arange(case.n)
        x0, y0, w, h = (case.rect[:, j] for j in range(4))
        f = case.form
        us = np.stack([16 * x0 + 8 * w, 16 * y0 + 8 * h], 1).astype(np.float64)
        if case.policy == "gsplatcu":
            areas = np.stack([8 * w - 8, 8 * h - 8], 1)
            keyed = np.where(case.given, MIN_KEY, np.maximum(case.key.astype(np.int64), MIN_KEY))
            depths = depth_for_key(keyed)
            depths[f == FORM_NEAR] = F(0.1)
            m = f == FORM_OFF
            us[m] = np.stack([-100.0 - i % 50, np.full(n, 40.0)], 1)[m]
            areas[m] = 5
            m = f == FORM_EMPTY
            us[m] = np.stack([16 * x0, 16 * y0 + 8], 1)[m]
            areas[m] = 0
            m = f == FORM_REV
            us[m] = np.stack([16 * x0 + 8, 16 * y0 + 8], 1)[m]
            areas[m] = (-24, 0)
        else:
            areas = np.stack([8 * w - 1, 8 * h - 1], 1)
            depths = case.key.view(F).copy()
            depths[f == FORM_NEAR] = F(0.1)
            depths[f == FORM_REV] = F(150.0)
            depths[(f == FORM_OFF) | (f == FORM_EMPTY)] = F(1.5)
            m = f == FORM_OFF
            us[m] = (-1.5 * case.W, -1.5 * case.H)
            m = f == FORM_EMPTY
            us[m] = (-50.0, -50.0)
            areas[m] = 3
        if case.depth is not None:
            depths = np.where(case.given, case.depth, depths).astype(F)
        case._built = (np.ascontiguousarray(us, F), np.ascontiguousarray(areas, np.int32), np.ascontiguousarray(depths, F))
    return tuple(a.copy() for a in case._built)


def reference_lists(case):
    """-> dict: ranges [T, 2] int32 ((0, 0) for empty tiles), ids [P] int32, P, maxkey (largest key among the Gaussians
    with patches, 0 without any), depths / areas after the in-place cull, visible [n] uint8 (depth > 0.2 after it)"""
    if case._ref is not None:
        return case._ref
    gx, gy = grid(case.W, case.H)
    has = np.nonzero(case.form == FORM_PATCH)[0]                  # index order
    x0, y0 = case.rect[has, 0], case.rect[has, 1]
    x1, y1 = x0 + case.rect[has, 2], y0 + case.rect[has, 3]
    key = case.key[has]
    ranges = np.zeros((gx * gy, 2), np.int32)
    chunks, p = [], 0
    for ty in range(gy):
        rows = np.nonzero((y0 <= ty) & (ty < y1))[0]
        if rows.size == 0:
            continue
        rx0, rx1 = x0[rows], x1[rows]
        cover = np.cumsum(np.bincount(rx0, minlength=gx + 1) - np.bincount(rx1, minlength=gx + 1))[:gx]
        for tx in np.nonzero(cover > 0)[0]:
            m = rows[(rx0 <= tx) & (tx < rx1)]                     # the Gaussians whose rect contains the tile, by index
            m = m[np.argsort(key[m], kind="stable")]               # ... by (key, index)
            ranges[ty * gx + tx] = (p, p + m.size)
            chunks.append(has[m])
            p += m.size
    ids = np.concatenate(chunks).astype(np.int32) if chunks else np.zeros(0, np.int32)
    us, areas, depths = build(case)
    if case.policy == "gsplatcu":
        culled = case.form >= FORM_OFF
        depths[culled] = F(-1.0)
        areas[culled] = 0
    with np.errstate(invalid="ignore"):
        visible = (depths > F(0.2)).astype(np.uint8)
    case._ref = dict(ranges=ranges, ids=ids, P=p, maxkey=int(key.max()) if key.size else 0, depths=depths, areas=areas,
                     visible=visible)
    return case._ref


def sorted_has(case):
    """[n] bool: does the Gaussian at position j of the DEPTH order have patches (what k_bin_scan_* / k_bin_emit see)"""
    has = case.form == FORM_PATCH
    k = np.where(has, case.key, 0)
    return has[np.argsort(k, kind="stable")]


# ------------------------------------------------------------------------------------------------------------ the sets
def _hash(i, mod):
    return (np.asarray(i, np.int64) * 2654435761 % (1 << 32)) % mod


def _zero_forms(zero):
    """forms of the Gaussians: the patch-less ones rotate through the four ways of having none"""
    zero = np.asarray(zero, bool)
    return np.where(zero, 1 + (np.cumsum(zero) - 1) % 4, FORM_PATCH)


COUNT_N = (1, 2, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4097)
COUNT_PATTERNS = ("all", "first_of_wg", "last_of_wg", "empty_wg", "only_last", "only_first", "none")
COUNT_WHAT = {"all": "every Gaussian one tile", "first_of_wg": "the first Gaussian of every 256 without patches",
              "last_of_wg": "the last Gaussian of every 256 (and of the partial one) without patches",
              "empty_wg": "every second run of 256 Gaussians without patches", "only_last": "only the last with patches",
              "only_first": "only the first with patches", "none": "no Gaussian with patches: P == 0 with n > 0"}


def count_zero(n, pattern):
    i = np.arange(n)
    return {"all": np.zeros(n, bool), "first_of_wg": i % WG == 0, "last_of_wg": (i % WG == WG - 1) | (i == n - 1),
            "empty_wg": (i // WG) % 2 == 1, "only_last": i != n - 1, "only_first": i != 0,
            "none": np.ones(n, bool)}[pattern]


def _counts():
    out = []
    W, H = 150, 70                                          # 10 x 5 tiles, partial tiles on both edges
    for n in COUNT_N:
        i = np.arange(n)
        t = (i * 7) % 50
        rect = np.stack([t % 10, t // 10, np.ones(n, np.int64), np.ones(n, np.int64)], 1)
        for pattern in COUNT_PATTERNS:
            zero = count_zero(n, pattern)
            P = int((~zero).sum())
            for mode in ("mm", "nan"):
                if mode == "nan" and pattern == "none":
                    continue
                form = _zero_forms(zero)
                props = [("zero_index" if z else "patch_index", int(j)) for j, z in enumerate(zero)
                         if j % WG in (0, WG - 1) or j == n - 1]
                if mode == "mm":
                    key = MIN_KEY + _hash(i, 97)
                    depth = given = None
                    if zero.any() and not zero.all():       # the depth sort moves the patch-less ones to the front
                        nz = int(zero.sum())
                        props += [("zero_sorted", nz - 1), ("patch_sorted", nz)]
                else:                                       # every key 0: depth order == index order
                    key = np.zeros(n, np.uint32)
                    depth, given = np.full(n, np.nan, F), ~zero
                    props += [("zero_sorted" if z else "patch_sorted", int(j)) for j, z in enumerate(zero)
                              if j % WG in (0, WG - 1) or j == n - 1]
                out.append(Case("n%d_%s_%s" % (n, pattern, mode), "counts", "gsplatcu", W, H, rect, key, form,
                                COUNT_WHAT[pattern] + (", keys >= 200" if mode == "mm" else ", every depth NaN (key 0)"),
                                dict(n=n, P=P), props, depth, given))
    # one Gaussian whose run is longer than a workgroup of k_bin_emit, alone among patch-less ones
    n = 300
    rect = np.tile([3, 2, 1, 1], (n, 1))
    rect[130] = (0, 0, 20, 15)
    out.append(Case("one_big_alone", "counts", "gsplatcu", 320, 240, rect, np.full(n, 4321), _zero_forms(np.arange(n) != 130),
                    "one Gaussian over 20 x 15 tiles (EGS_CR_BIG, not cullable on the tensor surface) among patch-less ones",
                    dict(n=n, P=300, depth_passes=2), [("span_over", WG), ("patch_index", 130), ("zero_sorted", n - 2),
                                                       ("patch_sorted", n - 1)]))
    # rects on both sides of the bitmap / big border (4 x 4 tiles), side by side and stacked with an offset
    rows = []
    for r in range(2):
        rows += [(0, r, 4, 4), (4, r, 4, 5), (8, r, 5, 4), (13, r, 1, 9), (14, r, 4, 4)]
    rows += [(3, 3, 1, 1)] * 3
    rect = np.array(rows)
    n = len(rows)
    form = np.zeros(n, np.int64)
    form[-2] = FORM_EMPTY
    P = int(sum(w * h for (_, _, w, h), f in zip(rows, form) if f == FORM_PATCH))
    out.append(Case("bitmap_border", "counts", "gsplatcu", 320, 160, rect, 900 - 7 * np.arange(n), form,
                    "rects of 4x4, 4x5, 5x4 and 1x9 tiles side by side: both sides of the bitmap / big border",
                    dict(n=n, P=P, depth_passes=2), [("count_is", 0, 16), ("count_is", 1, 20), ("count_is", 2, 20),
                                                     ("count_is", 3, 9)]))
    return out


TOTAL_P = (3, 4, 5, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 2049, 4095, 4096, 4097)


def spread_first_run(P):
    """length of tile 0's run in the ``spread`` cases: the largest k_tile_ranges workgroup border (also the sort-tile
    border at 2048 and 4096) below P, else the largest quad border below P, else 1"""
    if P > RANGE_WG:
        return RANGE_WG * ((P - 1) // RANGE_WG)
    return QUAD * ((P - 1) // QUAD) if P > QUAD else 1


def _totals():
    out = []
    W, H = 64, 48                                           # 4 x 3 tiles
    for P in TOTAL_P:
        i = np.arange(P)
        out.append(Case("P%d_one_tile" % P, "totals", "gsplatcu", W, H, np.tile([1, 1, 1, 1], (P, 1)),
                        MIN_KEY + _hash(i, 97), np.zeros(P), "every patch in tile 5", dict(n=P, P=P),
                        [("run_end", P), ("tile_len", 5, P)]))
        L0 = spread_first_run(P)
        rem = P - L0
        tiles = np.concatenate([np.zeros(L0, np.int64), np.full(max(rem - 1, 0), 2), np.full(1 if rem >= 1 else 0, 11)])
        tiles = tiles[np.random.RandomState(P).permutation(P)]
        n = P + (P + 3) // 4                                # a patch-less Gaussian in front of every four others
        zero = np.arange(n) % 5 == 0
        assert int((~zero).sum()) == P
        t = np.zeros(n, np.int64)
        t[~zero] = tiles
        rect = np.stack([t % 4, t // 4, np.ones(n, np.int64), np.ones(n, np.int64)], 1)
        props = [("run_end", L0), ("tile_len", 0, L0), ("tile_len", 1, 0), ("tile_len", 11, 1)]
        if rem >= 2:
            props.append(("run_end", P - 1))
        out.append(Case("P%d_spread" % P, "totals", "gsplatcu", W, H, rect, MIN_KEY + _hash(np.arange(n), 97),
                        _zero_forms(zero), "tile 0's run ends on the border %d, tile 1 is empty, the last tile holds "
                        "the last patch" % L0, dict(n=n, P=P), props))
    return out


KEYS_N = 3000
KEY_MAXES = (255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)


def _keys_geometry():
    n, i = KEYS_N, np.arange(KEYS_N)
    t = (i * 5) % 12
    x0, y0 = t % 4, t // 4
    two = (i % 11 == 0) & (x0 <= 2) & (y0 <= 1)
    rect = np.stack([x0, y0, np.where(two, 2, 1), np.where(two, 2, 1)], 1)
    return n, i, rect, _zero_forms(i % 13 == 0)


def _keys():
    out = []
    n, i, rect, form = _keys_geometry()
    W, H = 64, 48
    G = lambda name, key, what, passes, **kw: out.append(
        Case(name, "keys", "gsplatcu", W, H, kw.pop("rect", rect), key, form, what,
             dict(n=n, depth_passes=passes, maxkey=kw.pop("maxkey")), **kw))
    G("equal", np.full(n, 777), "all keys equal: index order inside every tile", 2, maxkey=777)
    G("descending", MIN_KEY + (n - 1 - i), "keys strictly descending by index", 2,
      maxkey=int((MIN_KEY + (n - 1 - i))[form == FORM_PATCH].max()))
    for K in KEY_MAXES:
        top = min(K, 1 << 22)                               # (see depth_for_key: not every key above 2^23 exists)
        key = MIN_KEY + _hash(i, top - MIN_KEY)
        key[1500] = K
        G("max%d" % K, key, "keys in [200, %d), one key %d: %d significant bits" % (top, K, bit_length(K)),
          sort_passes(bit_length(K)), maxkey=K)
    # keys that saturate or vanish: 5e6 * 1000 and +inf convert to 0xFFFFFFFF, NaN to 0 (all three keep their patches)
    key = MIN_KEY + _hash(i, 65535 - MIN_KEY)
    depth, given = np.zeros(n, F), np.zeros(n, bool)
    r2 = rect.copy()
    for j, (d, k) in {100: (5e6, SAT), 200: (np.inf, SAT), 300: (np.nan, 0), 1700: (np.inf, SAT), 1701: (5e6, SAT)}.items():
        depth[j], given[j], key[j] = d, True, k
        r2[j] = (1, 1, 1, 1)
        assert form[j] == FORM_PATCH
    G("saturate", key, "depths 5e6 and +inf (key 0xFFFFFFFF, ties by index) and NaN (key 0) in tile 5", 4, maxkey=SAT,
      rect=r2, depth=depth, given=given)
    # forward_cpu: the float bits are the key; all four passes are real
    A = lambda name, bits, what: out.append(
        Case(name, "keys", "forward_cpu", W, H, rect, bits, form, what,
             dict(n=n, depth_passes=4, maxkey=int(np.asarray(bits, np.uint32)[form == FORM_PATCH].max()))))
    A("f32_top", ((0x3E + i % 5) << 24) | 0x800000, "float-bit keys that differ in the top byte only (0.25 .. 64)")
    A("f32_bottom", 0x3F800000 | _hash(i, 256), "float-bit keys that differ in the bottom byte only (1.0 ..)")
    A("f32_all", (F(0.25) + F(89.0) * ((i * 0.6180339887498949) % 1.0).astype(F)).astype(F).view(np.uint32),
      "float-bit keys that differ in all four bytes (0.25 .. 89.25)")
    return out


GRIDS = ((13, 9), (20, 11), (265, 235), (250, 249), (4109, 9), (2040, 1020), (2056, 1017))
GRID_BIG = (4100, 4101)                                     # 257 x 257 = 66 049 tiles: 17 bits, three passes
GRID_BITS = {1: 1, 2: 1, 255: 8, 256: 8, 257: 9, 8192: 13, 8256: 14, 66049: 17}


def _grid_case(W, H):
    gx, gy = grid(W, H)
    T = gx * gy
    n, i = 300, np.arange(300)
    t = _hash(i, T)
    x0, y0 = t % gx, t // gx
    col, row = (i >= 2) & (i < 40) & (i % 2 == 0), (i >= 2) & (i < 40) & (i % 2 == 1)
    x0, y0 = np.where(col, gx - 1, x0), np.where(col, i % gy, y0)
    x0, y0 = np.where(row, i % gx, x0), np.where(row, gy - 1, y0)
    x0[0], y0[0] = 0, 0
    x0[1], y0[1] = gx - 1, gy - 1
    two = (i % 9 == 0) & (x0 < gx - 1) & (y0 < gy - 1) & (i > 1)
    rect = np.stack([x0, y0, np.where(two, 2, 1), np.where(two, 2, 1)], 1)
    zero = (i % 17 == 5)
    bits = tile_key_bits(T)
    return Case("T%d" % T, "grid", "gsplatcu", W, H, rect, MIN_KEY + _hash(i, 4801), _zero_forms(zero),
                "%d x %d tiles (%d x %d pixels): a %d-bit tile key, passes of %s bits" % (gx, gy, W, H, bits, pass_widths(bits)),
                dict(n=n, T=T, tile_key_bits=GRID_BITS[T], tile_passes=sort_passes(GRID_BITS[T]), depth_passes=2),
                [("tile_has", 0), ("tile_has", T - 1), ("column_has", gx - 1), ("row_has", gy - 1)])


def _grid():
    return [_grid_case(W, H) for W, H in GRIDS + (GRID_BIG,)]


LARGE_N = (RS_SHORT, RS_SHORT + 1)


def large_case(n):
    """one tile each on 64 x 64 tiles, keys from a fixed permutation of 3000 values, every 7th without patches"""
    i = np.arange(n)
    t = _hash(i, 4096)
    rect = np.stack([t % 64, t // 64, np.ones(n, np.int64), np.ones(n, np.int64)], 1)
    perm = np.random.RandomState(20).permutation(3000)
    zero = i % 7 == 3
    return Case("n%d" % n, "large", "gsplatcu", 1024, 1024, rect, MIN_KEY + perm[_hash(i + 11, 3000)], _zero_forms(zero),
                "%d Gaussians: the %s items-per-thread instances of the depth sort" % (n, "8" if n <= RS_SHORT else "16"),
                dict(n=n, P=n - int(zero.sum()), depth_passes=2, sort_ipt=8 if n <= RS_SHORT else 16))


_SETS = {"counts": _counts, "totals": _totals, "keys": _keys, "grid": _grid}
_cache = {}


def cases(cset):
    """the cases of a set (built once; ``large`` is built one case at a time by large_case)"""
    if cset not in _cache:
        _cache[cset] = _SETS[cset]()
    return _cache[cset]


def names(cset):
    return [c.name for c in cases(cset)]


def get(cset, name):
    return next(c for c in cases(cset) if c.name == name)
