// libegs_simplify.so (include/egs_simplify.h, which states every rule): vertex-clustering simplification of an indexed
// triangle mesh with quadric-optimal representatives.  Every kernel walks its items with the stride of a
// capped grid.
//
//   k_keys            : a thread per vertex: the 3 x 21-bit cell key
//   k_vertex_quadrics : a thread per vertex walks its incidence row and writes the 9 doubles of its plane quadric (the
//                       vertex-parallel pass of the two-pass form: a long row costs one thread, not a whole cluster)
//   k_clusters        : a thread per cluster sums its members in ascending order -- their stored quadrics, or, without that
//                       buffer, each member's quadric formed on the spot by the same device function (fused form: the same
//                       additions in the same order, the same bits) --, solves the regularised 3 x 3 system by a Cholesky
//                       factorisation written out, clamps to the cell, rounds once
//   k_remap_faces     : a thread per face: corners through cluster[], rotation, validity, the 2 x int64 sort key
//   k_clear_flags, k_first_of_run : fkeep and ckeep zeroed, then a thread per SORTED position sets fkeep of the first face of
//                       each run of equal keys and ckeep of its three clusters (plain stores of the value 1)
//
// These are gathers bound by dependent loads, not by arithmetic.  No thread waits for another, no LDS, no atomic: every
// output is a pure function of the input.  All double arithmetic is compiled without contraction.
#define EGS_SIDE_LIBRARY "egs_simplify"
#include "egs_side_error.h"

#include <math.h>

#include <initializer_list>

#include "../../include/egs_simplify.h"

static_assert(EGS_SIMPLIFY_ERR_BAD_ARG == EGS_ERR_BAD_ARG, "one bad-argument code across the libraries");

#pragma clang fp contract(off)

namespace egs {

constexpr int SF_THREADS = 256;
constexpr int64_t SF_INDEX_MAX = ((int64_t)1 << EGS_SIMPLIFY_KEY_BITS) - 1;
constexpr double SF_DBL_MAX = 1.7976931348623157e308;
constexpr double SF_RHO = 1e-3;

// the stride walk: item i of n for this thread
#define SF_WALK(i, n)                                                                                       \
  for (int64_t i = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x, n__ = (int64_t)(n),                      \
               step__ = (int64_t)gridDim.x * SF_THREADS;                                                    \
       i < n__; i += step__)

// the three indices of face f -> false if one lies outside [0, V)
__device__ __forceinline__ bool load_face(const int64_t* __restrict__ faces, int64_t f, int V, int& a, int& b, int& c) {
  const int64_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  a = (int)ia; b = (int)ib; c = (int)ic;
  return ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V;
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ld3(const float* __restrict__ p, int64_t i) {
  return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]};
}

struct Origin { double x, y, z, cell; };

__device__ __forceinline__ int64_t cell_index(double p, double o, double cell) {
  const double q = floor((p - o) / cell);
  return q >= 0.0 ? (q <= (double)SF_INDEX_MAX ? (int64_t)q : SF_INDEX_MAX) : 0;      // (NaN fails q >= 0)
}

// the centre of the cell a key names; whatever the key's bits, three indices in [0, 2^21)
__device__ __forceinline__ D3 key_centre(int64_t key, const Origin& o) {
  const int64_t ix = key & SF_INDEX_MAX, iy = (key >> EGS_SIMPLIFY_KEY_BITS) & SF_INDEX_MAX,
                iz = (key >> (2 * EGS_SIMPLIFY_KEY_BITS)) & SF_INDEX_MAX;
  return {o.x + ((double)ix + 0.5) * o.cell, o.y + ((double)iy + 0.5) * o.cell, o.z + ((double)iz + 0.5) * o.cell};
}

__global__ __launch_bounds__(SF_THREADS) void k_keys(int V, const float* __restrict__ vertices, Origin o,
                                                     int64_t* __restrict__ keys) {
  SF_WALK(v, V) {
    const D3 p = ld3(vertices, v);
    const int64_t ix = cell_index(p.x, o.x, o.cell), iy = cell_index(p.y, o.y, o.cell), iz = cell_index(p.z, o.z, o.cell);
    keys[v] = ix | (iy << EGS_SIMPLIFY_KEY_BITS) | (iz << (2 * EGS_SIMPLIFY_KEY_BITS));
  }
}

struct Q9 { double q[9]; };      // a00 a01 a02 a11 a12 a22 g0 g1 g2

// the plane quadric of vertex v about the centre c of its cell: its incidence row in row order
__device__ __forceinline__ Q9 vertex_quadric(int V, int F, const float* __restrict__ vertices,
                                             const int64_t* __restrict__ faces, const int64_t* __restrict__ row_start,
                                             const int64_t* __restrict__ rows, int64_t v, const D3& c) {
  Q9 s;
#pragma unroll
  for (int k = 0; k < 9; ++k) s.q[k] = 0.0;
  if (F <= 0) return s;
  const int64_t entries = 3 * (int64_t)F;
  int64_t e0 = row_start[v], e1 = row_start[v + 1];
  e0 = e0 < 0 ? 0 : e0;
  e1 = e1 > entries ? entries : e1;
  for (int64_t i = e0; i < e1; ++i) {
    const int64_t e = rows[i];
    if (e < 0 || e >= entries) continue;
    int ia, ib, ic;
    if (!load_face(faces, e / 3, V, ia, ib, ic)) continue;
    const D3 A = ld3(vertices, ia), B = ld3(vertices, ib), C = ld3(vertices, ic);
    const double ux = B.x - A.x, uy = B.y - A.y, uz = B.z - A.z;
    const double wx = C.x - A.x, wy = C.y - A.y, wz = C.z - A.z;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double L = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(L > 0.0 && L <= SF_DBL_MAX)) continue;
    const double inv = 1.0 / L;
    const double mx = inv * nx, my = inv * ny, mz = inv * nz;
    const double rx = A.x - c.x, ry = A.y - c.y, rz = A.z - c.z;
    const double d = (nx * rx + ny * ry) + nz * rz;
    s.q[0] += mx * nx; s.q[1] += mx * ny; s.q[2] += mx * nz;
    s.q[3] += my * ny; s.q[4] += my * nz; s.q[5] += mz * nz;
    s.q[6] += d * mx;  s.q[7] += d * my;  s.q[8] += d * mz;
  }
  return s;
}

__global__ __launch_bounds__(SF_THREADS) void k_vertex_quadrics(int V, int F, const float* __restrict__ vertices,
                                                                const int64_t* __restrict__ faces,
                                                                const int64_t* __restrict__ row_start,
                                                                const int64_t* __restrict__ rows,
                                                                const int64_t* __restrict__ keys, Origin o,
                                                                double* __restrict__ quadrics) {
  SF_WALK(v, V) {
    const Q9 s = vertex_quadric(V, F, vertices, faces, row_start, rows, v, key_centre(keys[v], o));
#pragma unroll
    for (int k = 0; k < 9; ++k) quadrics[9 * v + k] = s.q[k];
  }
}

__device__ __forceinline__ double clamp_to(double y, double h, bool& clamped) {
  if (y < -h) { clamped = true; return -h; }
  if (y > h) { clamped = true; return h; }
  return y;
}

__global__ __launch_bounds__(SF_THREADS) void k_clusters(int V, int F, int Vc, const float* __restrict__ vertices,
                                                         const float* __restrict__ colors,
                                                         const int64_t* __restrict__ keys,
                                                         const int64_t* __restrict__ member_start,
                                                         const int64_t* __restrict__ members,
                                                         const double* __restrict__ quadrics,
                                                         const int64_t* __restrict__ faces,
                                                         const int64_t* __restrict__ row_start,
                                                         const int64_t* __restrict__ rows, Origin o, int placement,
                                                         float* __restrict__ out_vertices, float* __restrict__ out_colors,
                                                         int32_t* __restrict__ placed) {
  const bool quadric = placement == EGS_SIMPLIFY_PLACE_QUADRIC;
  SF_WALK(ci, Vc) {
    int64_t m0 = member_start[ci], m1 = member_start[ci + 1];
    m0 = m0 < 0 ? 0 : m0;
    m1 = m1 > V ? V : m1;
    Q9 S;
#pragma unroll
    for (int k = 0; k < 9; ++k) S.q[k] = 0.0;
    double sx = 0.0, sy = 0.0, sz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
    D3 c = key_centre(0, o);
    int64_t count = 0;
    for (int64_t i = m0; i < m1; ++i) {
      const int64_t v = members[i];
      if (v < 0 || v >= V) continue;
      const int64_t key = keys[v];
      if (count == 0) c = key_centre(key, o);
      ++count;
      const D3 p = ld3(vertices, v);
      sx += p.x - c.x; sy += p.y - c.y; sz += p.z - c.z;
      if (colors) {
        const D3 col = ld3(colors, v);
        cr += col.x; cg += col.y; cb += col.z;
      }
      if (quadric) {
        if (quadrics) {
#pragma unroll
          for (int k = 0; k < 9; ++k) S.q[k] += quadrics[9 * v + k];
        } else {
          const Q9 s = vertex_quadric(V, F, vertices, faces, row_start, rows, v, key_centre(key, o));
#pragma unroll
          for (int k = 0; k < 9; ++k) S.q[k] += s.q[k];
        }
      }
    }
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    int what = quadric ? 3 : 0;
    if (count > 0) {
      const double n = (double)count;
      const double mx = sx / n, my = sy / n, mz = sz / n;
      cr = cr / n; cg = cg / n; cb = cb / n;
      y0 = mx; y1 = my; y2 = mz;
      const double tr = (S.q[0] + S.q[3]) + S.q[5];
      if (quadric && tr > 0.0 && tr <= SF_DBL_MAX) {
        const double rho = SF_RHO * tr;
        const double b00 = S.q[0] + rho, b01 = S.q[1], b02 = S.q[2], b11 = S.q[3] + rho, b12 = S.q[4], b22 = S.q[5] + rho;
        const double r0 = S.q[6] + rho * mx, r1 = S.q[7] + rho * my, r2 = S.q[8] + rho * mz;
        const double l00 = sqrt(b00), l10 = b01 / l00, l20 = b02 / l00;
        const double l11 = sqrt(b11 - l10 * l10), l21 = (b12 - l20 * l10) / l11;
        const double l22 = sqrt((b22 - l20 * l20) - l21 * l21);
        const double z0 = r0 / l00, z1 = (r1 - l10 * z0) / l11, z2 = ((r2 - l20 * z0) - l21 * z1) / l22;
        y2 = z2 / l22;
        y1 = (z1 - l21 * y2) / l11;
        y0 = ((z0 - l10 * y1) - l20 * y2) / l00;
        what = 1;
      }
      if (quadric) {
        bool clamped = false;
        const double h = 0.5 * o.cell;
        y0 = clamp_to(y0, h, clamped); y1 = clamp_to(y1, h, clamped); y2 = clamp_to(y2, h, clamped);
        if (clamped && what == 1) what = 2;
      }
    }
    out_vertices[3 * ci] = (float)(c.x + y0);
    out_vertices[3 * ci + 1] = (float)(c.y + y1);
    out_vertices[3 * ci + 2] = (float)(c.z + y2);
    if (colors) {
      out_colors[3 * ci] = (float)cr; out_colors[3 * ci + 1] = (float)cg; out_colors[3 * ci + 2] = (float)cb;
    }
    placed[ci] = what;
  }
}

__global__ __launch_bounds__(SF_THREADS) void k_remap_faces(int V, int F, int Vc, const int64_t* __restrict__ faces,
                                                            const int64_t* __restrict__ cluster,
                                                            int64_t* __restrict__ rotated, int32_t* __restrict__ valid,
                                                            int64_t* __restrict__ key_hi, int64_t* __restrict__ key_lo) {
  SF_WALK(f, F) {
    int ia, ib, ic;
    int64_t a = -1, b = -1, c = -1;
    bool ok = load_face(faces, f, V, ia, ib, ic);
    if (ok) {
      a = cluster[ia]; b = cluster[ib]; c = cluster[ic];
      ok = a >= 0 && a < Vc && b >= 0 && b < Vc && c >= 0 && c < Vc && a != b && b != c && a != c;
    }
    if (ok) {
      if (b < a && b < c) { const int64_t t = a; a = b; b = c; c = t; }           // (a, b, c) -> (b, c, a)
      else if (c < a && c < b) { const int64_t t = a; a = c; c = b; b = t; }      // (a, b, c) -> (c, a, b)
    } else {
      a = b = c = -1;
    }
    rotated[3 * f] = a; rotated[3 * f + 1] = b; rotated[3 * f + 2] = c;
    valid[f] = ok ? 1 : 0;
    key_hi[f] = ok ? a * (int64_t)Vc + b : -1;
    key_lo[f] = c;
  }
}

__global__ __launch_bounds__(SF_THREADS) void k_clear_flags(int F, int Vc, int32_t* __restrict__ fkeep,
                                                            int32_t* __restrict__ ckeep) {
  SF_WALK(f, F) fkeep[f] = 0;
  SF_WALK(c, Vc) ckeep[c] = 0;
}

__global__ __launch_bounds__(SF_THREADS) void k_first_of_run(int F, int Vc, const int64_t* __restrict__ order,
                                                             const int64_t* __restrict__ rotated,
                                                             const int32_t* __restrict__ valid,
                                                             const int64_t* __restrict__ key_hi,
                                                             const int64_t* __restrict__ key_lo, int32_t* fkeep,
                                                             int32_t* ckeep) {
  SF_WALK(i, F) {
    const int64_t f = order[i];
    if (f < 0 || f >= F || valid[f] == 0) continue;
    bool first = i == 0;
    if (!first) {
      const int64_t p = order[i - 1];
      first = p < 0 || p >= F || key_hi[p] != key_hi[f] || key_lo[p] != key_lo[f];
    }
    if (!first) continue;
    fkeep[f] = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t r = rotated[3 * f + k];
      if (r >= 0 && r < Vc) ckeep[r] = 1;      // (every writer stores the same value)
    }
  }
}

}  // namespace egs

using namespace egs;

static bool aligned_to(const void* a, uintptr_t k) { return ((uintptr_t)a & (k - 1)) == 0; }
static bool blocks_ok(int max_blocks) { return max_blocks >= 0 && max_blocks <= EGS_SIMPLIFY_MAX_BLOCKS; }
static bool is_finite(double x) { return fabs(x) <= SF_DBL_MAX; }      // (false for NaN)
static bool grid_ok(double ox, double oy, double oz, double cell) {
  return is_finite(ox) && is_finite(oy) && is_finite(oz) && is_finite(cell) && cell > 0.0;
}
static int grid_for(int64_t items, int max_blocks) {
  const int64_t cap = max_blocks > 0 ? max_blocks : EGS_SIMPLIFY_MAX_BLOCKS;
  const int64_t want = (items + SF_THREADS - 1) / SF_THREADS;
  return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}
// no two of the non-null pointers are equal
static bool distinct(std::initializer_list<const void*> ps) {
  for (auto a = ps.begin(); a != ps.end(); ++a)
    for (auto b = a + 1; b != ps.end(); ++b)
      if (*a != nullptr && *a == *b) return false;
  return true;
}

extern "C" int egs_simplify_abi_version(void) { return EGS_SIMPLIFY_ABI_VERSION; }
extern "C" const char* egs_simplify_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_simplify_keys(int V, const float* vertices, double ox, double oy, double oz, double cell, int64_t* keys,
                                 int max_blocks, void* stream) {
  SIDE_CHECK_ARG(V >= 0);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(grid_ok(ox, oy, oz, cell));
  SIDE_CHECK_ARG(aligned_to(vertices, 4) && aligned_to(keys, 8));
  SIDE_CHECK_ARG(V == 0 || (vertices != nullptr && keys != nullptr));
  SIDE_CHECK_ARG(distinct({vertices, keys}));
  if (V == 0) return 0;
  hipLaunchKernelGGL(k_keys, dim3(grid_for(V, max_blocks)), dim3(SF_THREADS), 0, (hipStream_t)stream, V, vertices,
                     Origin{ox, oy, oz, cell}, keys);
  SIDE_HIP(hipGetLastError());
  return 0;
}

static bool incidence_ok(int V, int F, const int64_t* faces, const int64_t* row_start, const int64_t* rows) {
  return aligned_to(faces, 8) && aligned_to(row_start, 8) && aligned_to(rows, 8) &&
         (V == 0 || F == 0 || (faces != nullptr && row_start != nullptr && rows != nullptr));
}

extern "C" int egs_simplify_vertex_quadrics(int V, int F, const float* vertices, const int64_t* faces,
                                            const int64_t* row_start, const int64_t* rows, const int64_t* keys, double ox,
                                            double oy, double oz, double cell, double* quadrics, int max_blocks,
                                            void* stream) {
  SIDE_CHECK_ARG(V >= 0 && F >= 0);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(grid_ok(ox, oy, oz, cell));
  SIDE_CHECK_ARG(aligned_to(vertices, 4) && aligned_to(keys, 8) && aligned_to(quadrics, 8));
  SIDE_CHECK_ARG(incidence_ok(V, F, faces, row_start, rows));
  SIDE_CHECK_ARG(V == 0 || (vertices != nullptr && keys != nullptr && quadrics != nullptr));
  SIDE_CHECK_ARG(distinct({vertices, faces, row_start, rows, keys, quadrics}));
  if (V == 0) return 0;
  hipLaunchKernelGGL(k_vertex_quadrics, dim3(grid_for(V, max_blocks)), dim3(SF_THREADS), 0, (hipStream_t)stream, V, F,
                     vertices, faces, row_start, rows, keys, Origin{ox, oy, oz, cell}, quadrics);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_simplify_clusters(int V, int F, int Vc, const float* vertices, const float* colors, const int64_t* keys,
                                     const int64_t* member_start, const int64_t* members, const double* quadrics,
                                     const int64_t* faces, const int64_t* row_start, const int64_t* rows, double ox,
                                     double oy, double oz, double cell, int placement, float* out_vertices,
                                     float* out_colors, int32_t* placed, int max_blocks, void* stream) {
  SIDE_CHECK_ARG(V >= 0 && F >= 0 && Vc >= 0 && Vc <= V);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(grid_ok(ox, oy, oz, cell));
  SIDE_CHECK_ARG(placement == EGS_SIMPLIFY_PLACE_QUADRIC || placement == EGS_SIMPLIFY_PLACE_MEAN);
  SIDE_CHECK_ARG(aligned_to(vertices, 4) && aligned_to(colors, 4) && aligned_to(keys, 8) && aligned_to(member_start, 8) &&
                 aligned_to(members, 8) && aligned_to(quadrics, 8));
  SIDE_CHECK_ARG(aligned_to(faces, 8) && aligned_to(row_start, 8) && aligned_to(rows, 8));
  SIDE_CHECK_ARG(aligned_to(out_vertices, 4) && aligned_to(out_colors, 4) && aligned_to(placed, 4));
  const bool fused = placement == EGS_SIMPLIFY_PLACE_QUADRIC && quadrics == nullptr;
  SIDE_CHECK_ARG(Vc == 0 || (vertices != nullptr && keys != nullptr && member_start != nullptr && members != nullptr &&
                             out_vertices != nullptr && placed != nullptr && (colors == nullptr) == (out_colors == nullptr)));
  SIDE_CHECK_ARG(Vc == 0 || !fused || F == 0 || (faces != nullptr && row_start != nullptr && rows != nullptr));
  SIDE_CHECK_ARG(distinct({vertices, colors, keys, member_start, members, quadrics, faces, row_start, rows, out_vertices,
                           out_colors, placed}));
  if (Vc == 0) return 0;
  hipLaunchKernelGGL(k_clusters, dim3(grid_for(Vc, max_blocks)), dim3(SF_THREADS), 0, (hipStream_t)stream, V,
                     fused ? F : 0, Vc, vertices, colors, keys, member_start, members,
                     placement == EGS_SIMPLIFY_PLACE_QUADRIC ? quadrics : nullptr, faces, row_start, rows,
                     Origin{ox, oy, oz, cell}, placement, out_vertices, out_colors, placed);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_simplify_remap_faces(int V, int F, int Vc, const int64_t* faces, const int64_t* cluster,
                                        int64_t* rotated, int32_t* valid, int64_t* key_hi, int64_t* key_lo, int max_blocks,
                                        void* stream) {
  SIDE_CHECK_ARG(V >= 0 && F >= 0 && Vc >= 0 && Vc <= V);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(aligned_to(faces, 8) && aligned_to(cluster, 8) && aligned_to(rotated, 8) && aligned_to(valid, 4) &&
                 aligned_to(key_hi, 8) && aligned_to(key_lo, 8));
  SIDE_CHECK_ARG(F == 0 || (faces != nullptr && rotated != nullptr && valid != nullptr && key_hi != nullptr &&
                            key_lo != nullptr));
  SIDE_CHECK_ARG(F == 0 || V == 0 || cluster != nullptr);
  SIDE_CHECK_ARG(distinct({faces, cluster, rotated, valid, key_hi, key_lo}));
  if (F == 0) return 0;
  hipLaunchKernelGGL(k_remap_faces, dim3(grid_for(F, max_blocks)), dim3(SF_THREADS), 0, (hipStream_t)stream, V, F, Vc,
                     faces, cluster, rotated, valid, key_hi, key_lo);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_simplify_keep_flags(int F, int Vc, const int64_t* order, const int64_t* rotated, const int32_t* valid,
                                       const int64_t* key_hi, const int64_t* key_lo, int32_t* fkeep, int32_t* ckeep,
                                       int max_blocks, void* stream) {
  SIDE_CHECK_ARG(F >= 0 && Vc >= 0);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(aligned_to(order, 8) && aligned_to(rotated, 8) && aligned_to(valid, 4) && aligned_to(key_hi, 8) &&
                 aligned_to(key_lo, 8) && aligned_to(fkeep, 4) && aligned_to(ckeep, 4));
  SIDE_CHECK_ARG(F == 0 || (order != nullptr && rotated != nullptr && valid != nullptr && key_hi != nullptr &&
                            key_lo != nullptr && fkeep != nullptr));
  SIDE_CHECK_ARG(Vc == 0 || ckeep != nullptr);
  SIDE_CHECK_ARG(distinct({order, rotated, valid, key_hi, key_lo, fkeep, ckeep}));
  if (F == 0 && Vc == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_clear_flags, dim3(grid_for(F > Vc ? F : Vc, max_blocks)), dim3(SF_THREADS), 0, s, F, Vc, fkeep,
                     ckeep);
  if (F > 0)
    hipLaunchKernelGGL(k_first_of_run, dim3(grid_for(F, max_blocks)), dim3(SF_THREADS), 0, s, F, Vc, order, rotated, valid,
                       key_hi, key_lo, fkeep, ckeep);
  SIDE_HIP(hipGetLastError());
  return 0;
}
