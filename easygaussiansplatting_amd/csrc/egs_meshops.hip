// libegs_meshops.so (include/egs_meshops.h, which states every rule): cleaning of an indexed triangle mesh on the device
// (DESIGN 3.20).  Every kernel walks its items with the stride of a capped grid.
//
//   k_cc_init     : parent[v] = v (the label buffer IS the parent array), the two count arrays zeroed
//   k_cc_hook     : a thread per face unites (a, b) and (a, c): find both roots, atomicCAS the LARGER root's parent from
//                   itself to the smaller root, find again on a lost CAS.  parent[v] <= v throughout: no cycle, every
//                   retry means another thread made progress, and a component's root is its minimum index.  Finds halve
//                   their path (parent[v] <- an ancestor of v: safe under the same invariant).
//   k_cc_flatten  : label[v] = root(v), in place (every value written is a root, and a root's entry is never written)
//   k_cc_count    : integer atomics per representative; a wave whose active lanes all hold one label issues ONE add of
//                   their number (the usual mesh is one giant component: every add would land on one address)
//   k_keep_flags, k_compact : what is kept, and the scatter behind the caller's scans
//   k_vertex_normals, k_taubin_step : gathers over the vertex-to-face incidence, one thread per vertex, double sums in row
//                   order, no float atomic
//
// No thread waits for another, no LDS, no float atomic: every output is a pure function of the input.
#define EGS_SIDE_LIBRARY "egs_meshops"
#include "egs_side_error.h"

#include <math.h>

#include <initializer_list>

#include "../../include/egs_meshops.h"

static_assert(EGS_MESHOPS_ERR_BAD_ARG == EGS_ERR_BAD_ARG, "one bad-argument code across the libraries");

namespace egs {

constexpr int MO_THREADS = 256;
constexpr int MO_WAVE = 64;

// the stride walk: item i of n for this thread, every lane of a wave making the same number of trips (the bound is
// rounded up to whole waves), so wave-wide votes inside the loop see all their lanes
#define MO_WALK(i, n)                                                                                          \
  for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x,                                            \
               n_up__ = ((int64_t)(n) + MO_WAVE - 1) / MO_WAVE * MO_WAVE, step__ = (int64_t)gridDim.x * MO_THREADS; \
       i < n_up__; i += step__)

__device__ __forceinline__ int ld_parent(const int32_t* parent, int v) {
  return __atomic_load_n(parent + v, __ATOMIC_RELAXED);
}

// the root of v, halving the path on the way
__device__ __forceinline__ int cc_find(int32_t* parent, int v) {
  int p = ld_parent(parent, v);
  while (p != v) {
    const int g = ld_parent(parent, p);
    if (g != p) __atomic_store_n(parent + v, g, __ATOMIC_RELAXED);      // (v is no root and never becomes one again)
    v = p;
    p = g;
  }
  return v;
}

__device__ __forceinline__ void cc_unite(int32_t* parent, int a, int b) {
  for (;;) {
    const int ra = cc_find(parent, a), rb = cc_find(parent, b);
    if (ra == rb) return;
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
    a = hi;      // (hi was hooked by another thread meanwhile: look again from there)
    b = lo;
  }
}

// the three indices of face f -> false if one lies outside [0, V)
__device__ __forceinline__ bool load_face(const int64_t* __restrict__ faces, int64_t f, int V, int& a, int& b, int& c) {
  const int64_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  a = (int)ia; b = (int)ib; c = (int)ic;
  return ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V;
}

__global__ __launch_bounds__(MO_THREADS) void k_cc_init(int V, int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ comp_faces,
                                                        int32_t* __restrict__ comp_verts) {
  MO_WALK(v, V) {
    if (v < V) {
      parent[v] = (int32_t)v;
      comp_faces[v] = 0;
      comp_verts[v] = 0;
    }
  }
}

__global__ __launch_bounds__(MO_THREADS) void k_cc_hook(int V, int F, const int64_t* __restrict__ faces,
                                                        int32_t* parent) {
  MO_WALK(f, F) {
    int a, b, c;
    if (f < F && load_face(faces, f, V, a, b, c)) {
      if (a != b) cc_unite(parent, a, b);
      if (a != c) cc_unite(parent, a, c);
    }
  }
}

__global__ __launch_bounds__(MO_THREADS) void k_cc_flatten(int V, int32_t* label) {
  MO_WALK(v, V) {
    if (v < V) {
      int r = (int)v, p = ld_parent(label, r);
      while (p != r) {
        r = p;
        p = ld_parent(label, r);
      }
      if (r != (int)v) __atomic_store_n(label + v, r, __ATOMIC_RELAXED);
    }
  }
}

// one add of the wave's lane count when its active lanes agree, else one add per lane; every lane of the wave calls this
__device__ __forceinline__ void wave_count(int32_t* __restrict__ counts, bool active, int l) {
  const unsigned long long m = __ballot(active);
  if (m == 0) return;
  const int leader = __ffsll((long long)m) - 1;
  const int l0 = __shfl(l, leader, MO_WAVE);
  if (__ballot(active && l != l0) == 0) {
    if ((int)(threadIdx.x & (MO_WAVE - 1)) == leader) atomicAdd(counts + l0, __popcll(m));
  } else if (active) {
    atomicAdd(counts + l, 1);
  }
}

__global__ __launch_bounds__(MO_THREADS) void k_cc_count(int V, int F, const int64_t* __restrict__ faces,
                                                         const int32_t* __restrict__ label,
                                                         int32_t* __restrict__ comp_faces,
                                                         int32_t* __restrict__ comp_verts) {
  MO_WALK(v, V) {
    const bool on = v < V;
    wave_count(comp_verts, on, on ? label[v] : 0);
  }
  MO_WALK(f, F) {
    int a = 0, b, c;
    const bool on = f < F && load_face(faces, f, V, a, b, c);
    wave_count(comp_faces, on, on ? label[a] : 0);
  }
}

__global__ __launch_bounds__(MO_THREADS) void k_keep_flags(int V, int F, const int64_t* __restrict__ faces,
                                                           const int32_t* __restrict__ label,
                                                           const int32_t* __restrict__ comp_faces,
                                                           const int32_t* __restrict__ rank, int min_faces,
                                                           int keep_largest, int32_t* __restrict__ vkeep,
                                                           int32_t* __restrict__ fkeep) {
  auto kept = [&](int v) {
    const int r = label[v];
    if (r < 0 || r >= V) return false;
    return comp_faces[r] >= min_faces && (rank == nullptr || rank[r] < keep_largest);
  };
  MO_WALK(v, V) {
    if (v < V) vkeep[v] = kept((int)v) ? 1 : 0;
  }
  MO_WALK(f, F) {
    if (f < F) {
      int a, b, c;
      fkeep[f] = load_face(faces, f, V, a, b, c) && kept(a) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(MO_THREADS) void k_compact(int V, int F, const float* __restrict__ vertices,
                                                        const float* __restrict__ colors,
                                                        const float* __restrict__ normals,
                                                        const int64_t* __restrict__ faces,
                                                        const int32_t* __restrict__ vkeep,
                                                        const int32_t* __restrict__ fkeep,
                                                        const int64_t* __restrict__ vscan,
                                                        const int64_t* __restrict__ fscan, int Vk, int Fk,
                                                        float* __restrict__ out_vertices, float* __restrict__ out_colors,
                                                        float* __restrict__ out_normals, int64_t* __restrict__ out_faces) {
  MO_WALK(v, V) {
    if (v < V && vkeep[v] != 0) {
      const int64_t d = vscan[v] - 1;
      if (d >= 0 && d < Vk) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          out_vertices[3 * d + k] = vertices[3 * v + k];
          if (colors) out_colors[3 * d + k] = colors[3 * v + k];
          if (normals) out_normals[3 * d + k] = normals[3 * v + k];
        }
      }
    }
  }
  MO_WALK(f, F) {
    if (f < F && fkeep[f] != 0) {
      const int64_t d = fscan[f] - 1;
      int a, b, c;
      if (d >= 0 && d < Fk && load_face(faces, f, V, a, b, c)) {
        out_faces[3 * d] = vscan[a] - 1;
        out_faces[3 * d + 1] = vscan[b] - 1;
        out_faces[3 * d + 2] = vscan[c] - 1;
      }
    }
  }
}

// the row of vertex v, clipped to the entries the buffer has
__device__ __forceinline__ void row_of(const int64_t* __restrict__ row_start, int64_t v, int64_t entries, int64_t& e0,
                                       int64_t& e1) {
  e0 = row_start[v];
  e1 = row_start[v + 1];
  e0 = e0 < 0 ? 0 : e0;
  e1 = e1 > entries ? entries : e1;
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ld3(const float* __restrict__ p, int i) {
  return {(double)p[3 * (int64_t)i], (double)p[3 * (int64_t)i + 1], (double)p[3 * (int64_t)i + 2]};
}

__global__ __launch_bounds__(MO_THREADS) void k_vertex_normals(int V, int F, const float* __restrict__ vertices,
                                                               const int64_t* __restrict__ faces,
                                                               const int64_t* __restrict__ row_start,
                                                               const int64_t* __restrict__ rows,
                                                               float* __restrict__ normals) {
#pragma clang fp contract(off)
  const int64_t entries = 3 * (int64_t)F;
  MO_WALK(v, V) {
    if (v >= V) continue;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (F > 0) {
      int64_t e0, e1;
      row_of(row_start, v, entries, e0, e1);
      for (int64_t i = e0; i < e1; ++i) {
        const int64_t e = rows[i];
        if (e < 0 || e >= entries) continue;
        int a, b, c;
        if (!load_face(faces, e / 3, V, a, b, c)) continue;
        const D3 A = ld3(vertices, a), B = ld3(vertices, b), C = ld3(vertices, c);
        const double ux = B.x - A.x, uy = B.y - A.y, uz = B.z - A.z;
        const double wx = C.x - A.x, wy = C.y - A.y, wz = C.z - A.z;
        sx += uy * wz - uz * wy;
        sy += uz * wx - ux * wz;
        sz += ux * wy - uy * wx;
      }
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool ok = len > 0.0 && len <= 1.7976931348623157e308;
    normals[3 * v] = ok ? (float)(sx / len) : 0.f;
    normals[3 * v + 1] = ok ? (float)(sy / len) : 0.f;
    normals[3 * v + 2] = ok ? (float)(sz / len) : 0.f;
  }
}

__global__ __launch_bounds__(MO_THREADS) void k_taubin_step(int V, int F, const float* __restrict__ src,
                                                            const int64_t* __restrict__ faces,
                                                            const int64_t* __restrict__ row_start,
                                                            const int64_t* __restrict__ rows, double s,
                                                            float* __restrict__ dst) {
#pragma clang fp contract(off)
  const int64_t entries = 3 * (int64_t)F;
  MO_WALK(v, V) {
    if (v >= V) continue;
    double ax = 0.0, ay = 0.0, az = 0.0;
    int64_t deg = 0;
    if (F > 0) {
      int64_t e0, e1;
      row_of(row_start, v, entries, e0, e1);
      for (int64_t i = e0; i < e1; ++i) {
        const int64_t e = rows[i];
        if (e < 0 || e >= entries) continue;
        int idx[3];
        if (!load_face(faces, e / 3, V, idx[0], idx[1], idx[2])) continue;
        const int k = (int)(e % 3);
        const D3 Q = ld3(src, idx[(k + 1) % 3]), R = ld3(src, idx[(k + 2) % 3]);
        ax += Q.x + R.x;
        ay += Q.y + R.y;
        az += Q.z + R.z;
        ++deg;
      }
    }
    const float px = src[3 * v], py = src[3 * v + 1], pz = src[3 * v + 2];
    if (deg == 0) {
      dst[3 * v] = px; dst[3 * v + 1] = py; dst[3 * v + 2] = pz;
    } else {
      const double den = 2.0 * (double)deg;
      dst[3 * v] = (float)((double)px + s * (ax / den - (double)px));
      dst[3 * v + 1] = (float)((double)py + s * (ay / den - (double)py));
      dst[3 * v + 2] = (float)((double)pz + s * (az / den - (double)pz));
    }
  }
}

__global__ __launch_bounds__(MO_THREADS) void k_copy_rows(int V, const float* __restrict__ src,
                                                          float* __restrict__ dst) {
  MO_WALK(i, 3 * (int64_t)V) {
    if (i < 3 * (int64_t)V) dst[i] = src[i];
  }
}

}  // namespace egs

using namespace egs;

static bool aligned_to(const void* a, uintptr_t k) { return ((uintptr_t)a & (k - 1)) == 0; }
static bool given(const void* p, uintptr_t k) { return p != nullptr && aligned_to(p, k); }
static bool blocks_ok(int max_blocks) { return max_blocks >= 0 && max_blocks <= EGS_MESHOPS_MAX_BLOCKS; }
static int grid_for(int64_t items, int max_blocks) {
  const int64_t cap = max_blocks > 0 ? max_blocks : EGS_MESHOPS_MAX_BLOCKS;
  const int64_t want = (items + MO_THREADS - 1) / MO_THREADS;
  return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}
// no two of the non-null pointers are equal
static bool distinct(std::initializer_list<const void*> ps) {
  for (auto a = ps.begin(); a != ps.end(); ++a)
    for (auto b = a + 1; b != ps.end(); ++b)
      if (*a != nullptr && *a == *b) return false;
  return true;
}

extern "C" int egs_meshops_abi_version(void) { return EGS_MESHOPS_ABI_VERSION; }
extern "C" const char* egs_meshops_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_meshops_components(int V, int F, const int64_t* faces, int32_t* label, int32_t* comp_faces,
                                      int32_t* comp_verts, int max_blocks, void* stream) {
  SIDE_CHECK_ARG(V >= 0 && F >= 0);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(aligned_to(faces, 8) && (F == 0 || faces != nullptr));
  SIDE_CHECK_ARG(aligned_to(label, 4) && aligned_to(comp_faces, 4) && aligned_to(comp_verts, 4));
  if (V == 0) return 0;
  SIDE_CHECK_ARG(label != nullptr && comp_faces != nullptr && comp_verts != nullptr);
  SIDE_CHECK_ARG(distinct({faces, label, comp_faces, comp_verts}));
  hipStream_t s = (hipStream_t)stream;
  const int gv = grid_for(V, max_blocks), gf = grid_for(F, max_blocks);
  hipLaunchKernelGGL(k_cc_init, dim3(gv), dim3(MO_THREADS), 0, s, V, label, comp_faces, comp_verts);
  if (F > 0) hipLaunchKernelGGL(k_cc_hook, dim3(gf), dim3(MO_THREADS), 0, s, V, F, faces, label);
  if (F > 0) hipLaunchKernelGGL(k_cc_flatten, dim3(gv), dim3(MO_THREADS), 0, s, V, label);
  hipLaunchKernelGGL(k_cc_count, dim3(gv > gf ? gv : gf), dim3(MO_THREADS), 0, s, V, F, faces, label, comp_faces,
                     comp_verts);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_meshops_keep_flags(int V, int F, const int64_t* faces, const int32_t* label,
                                      const int32_t* comp_faces, const int32_t* rank, int min_faces, int keep_largest,
                                      int32_t* vkeep, int32_t* fkeep, int max_blocks, void* stream) {
  SIDE_CHECK_ARG(V >= 0 && F >= 0);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(min_faces >= 0);
  SIDE_CHECK_ARG(keep_largest >= 0 && (keep_largest == 0 || V == 0 || rank != nullptr));
  SIDE_CHECK_ARG(aligned_to(faces, 8) && aligned_to(label, 4) && aligned_to(comp_faces, 4) && aligned_to(rank, 4) &&
                 aligned_to(vkeep, 4) && aligned_to(fkeep, 4));
  SIDE_CHECK_ARG(F == 0 || (faces != nullptr && fkeep != nullptr));
  SIDE_CHECK_ARG(V == 0 || (label != nullptr && comp_faces != nullptr && vkeep != nullptr));
  SIDE_CHECK_ARG(distinct({faces, label, comp_faces, rank, vkeep, fkeep}));
  if (V == 0 && F == 0) return 0;
  const int g = grid_for(V > F ? V : F, max_blocks);
  hipLaunchKernelGGL(k_keep_flags, dim3(g), dim3(MO_THREADS), 0, (hipStream_t)stream, V, F, faces, label, comp_faces,
                     keep_largest > 0 ? rank : nullptr, min_faces < 1 ? 1 : min_faces, keep_largest, vkeep, fkeep);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_meshops_compact(int V, int F, const float* vertices, const float* colors, const float* normals,
                                   const int64_t* faces, const int32_t* vkeep, const int32_t* fkeep, const int64_t* vscan,
                                   const int64_t* fscan, int Vk, int Fk, float* out_vertices, float* out_colors,
                                   float* out_normals, int64_t* out_faces, int max_blocks, void* stream) {
  SIDE_CHECK_ARG(V >= 0 && F >= 0);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(Vk >= 0 && Vk <= V && Fk >= 0 && Fk <= F);
  SIDE_CHECK_ARG(aligned_to(vertices, 4) && aligned_to(colors, 4) && aligned_to(normals, 4) && aligned_to(faces, 8) &&
                 aligned_to(vkeep, 4) && aligned_to(fkeep, 4) && aligned_to(vscan, 8) && aligned_to(fscan, 8));
  SIDE_CHECK_ARG(aligned_to(out_vertices, 4) && aligned_to(out_colors, 4) && aligned_to(out_normals, 4) &&
                 aligned_to(out_faces, 8));
  SIDE_CHECK_ARG(V == 0 || (vertices != nullptr && vkeep != nullptr && vscan != nullptr));
  SIDE_CHECK_ARG(F == 0 || (faces != nullptr && fkeep != nullptr && fscan != nullptr));
  SIDE_CHECK_ARG(Vk == 0 || (out_vertices != nullptr && (colors == nullptr) == (out_colors == nullptr) &&
                             (normals == nullptr) == (out_normals == nullptr)));
  SIDE_CHECK_ARG(Fk == 0 || (out_faces != nullptr && Vk > 0));
  SIDE_CHECK_ARG(distinct({vertices, colors, normals, faces, vkeep, fkeep, vscan, fscan, out_vertices, out_colors,
                           out_normals, out_faces}));
  if (Vk == 0) return 0;
  const int g = grid_for(V > F ? V : F, max_blocks);
  hipLaunchKernelGGL(k_compact, dim3(g), dim3(MO_THREADS), 0, (hipStream_t)stream, V, Fk > 0 ? F : 0, vertices,
                     out_colors ? colors : nullptr, out_normals ? normals : nullptr, faces, vkeep, fkeep, vscan, fscan, Vk,
                     Fk, out_vertices, out_colors, out_normals, out_faces);
  SIDE_HIP(hipGetLastError());
  return 0;
}

static bool incidence_ok(int V, int F, const float* vertices, const int64_t* faces, const int64_t* row_start,
                         const int64_t* rows) {
  return aligned_to(vertices, 4) && aligned_to(faces, 8) && aligned_to(row_start, 8) && aligned_to(rows, 8) &&
         (V == 0 || vertices != nullptr) && (V == 0 || F == 0 || (faces != nullptr && row_start != nullptr && rows != nullptr));
}

extern "C" int egs_meshops_vertex_normals(int V, int F, const float* vertices, const int64_t* faces,
                                          const int64_t* row_start, const int64_t* rows, float* normals, int max_blocks,
                                          void* stream) {
  SIDE_CHECK_ARG(V >= 0 && F >= 0);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(incidence_ok(V, F, vertices, faces, row_start, rows));
  SIDE_CHECK_ARG(aligned_to(normals, 4) && (V == 0 || normals != nullptr));
  SIDE_CHECK_ARG(distinct({vertices, faces, row_start, rows, normals}));
  if (V == 0) return 0;
  hipLaunchKernelGGL(k_vertex_normals, dim3(grid_for(V, max_blocks)), dim3(MO_THREADS), 0, (hipStream_t)stream, V, F,
                     vertices, faces, row_start, rows, normals);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_meshops_taubin(int V, int F, const float* vertices, const int64_t* faces, const int64_t* row_start,
                                  const int64_t* rows, int iterations, double lam, double mu, float* out, float* tmp,
                                  int max_blocks, void* stream) {
  SIDE_CHECK_ARG(V >= 0 && F >= 0);
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(iterations >= 0);
  SIDE_CHECK_ARG(fabs(lam) <= 1.7976931348623157e308 && fabs(mu) <= 1.7976931348623157e308);      // (false for NaN)
  SIDE_CHECK_ARG(incidence_ok(V, F, vertices, faces, row_start, rows));
  SIDE_CHECK_ARG(aligned_to(out, 4) && aligned_to(tmp, 4));
  SIDE_CHECK_ARG(V == 0 || (out != nullptr && (iterations == 0 || tmp != nullptr)));
  SIDE_CHECK_ARG(distinct({vertices, faces, row_start, rows, out, tmp}));
  if (V == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(V, max_blocks);
  if (iterations == 0) {
    hipLaunchKernelGGL(k_copy_rows, dim3(grid_for(3 * (int64_t)V, max_blocks)), dim3(MO_THREADS), 0, s, V, vertices, out);
  } else {
    const float* src = vertices;
    for (int it = 0; it < iterations; ++it) {      // lambda: src -> tmp, mu: tmp -> out
      hipLaunchKernelGGL(k_taubin_step, dim3(g), dim3(MO_THREADS), 0, s, V, F, src, faces, row_start, rows, lam, tmp);
      hipLaunchKernelGGL(k_taubin_step, dim3(g), dim3(MO_THREADS), 0, s, V, F, tmp, faces, row_start, rows, mu, out);
      src = out;
    }
  }
  SIDE_HIP(hipGetLastError());
  return 0;
}
