// What one lattice sample and one lattice cell of libegs_tsdf.so compute (include/egs_tsdf.h states the rules): plain
// functions of their arguments, host and device, so that csrc/egs_tsdf.hip's kernels are loops and memory traffic around
// them and a host program can call the same lines.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGS_HD __host__ __device__ __forceinline__
#else
#define EGS_HD inline
#endif

// every product and sum of this file is rounded on its own: the float32 restatement of the tests does the same, and an
// edge shared by several cells must give the same bits whichever expression the compiler would have fused
#pragma clang fp contract(off)

namespace egs_tsdf {

struct View {
  int H, W;
  float fx, fy, cx, cy;
  float R[9], t[3];
  float trunc, alpha_min, near, depth_max;
};

struct Lattice {
  int nx, ny, nz;
  float ox, oy, oz, voxel;
};

// Steps 1-5 of the header in two halves, so that a thread can have the gathers of its four samples in flight together.
// Steps 1-2 for the sample at lattice coordinates (ix, iy, iz): false = skipped (pix = 0: a pixel that can be read);
// otherwise its pixel and p_c.z
EGS_HD bool project_sample(const Lattice& L, const View& v, int ix, int iy, int iz, int& pix, float& pz) {
  const float x = L.ox + L.voxel * (float)ix, y = L.oy + L.voxel * (float)iy, z = L.oz + L.voxel * (float)iz;
  pz = ((v.R[6] * x + v.R[7] * y) + v.R[8] * z) + v.t[2];
  const float px = ((v.R[0] * x + v.R[1] * y) + v.R[2] * z) + v.t[0];
  const float py = ((v.R[3] * x + v.R[4] * y) + v.R[5] * z) + v.t[1];
  const float fu = floorf(((v.fx * px) / pz + v.cx) + 0.5f), fv = floorf(((v.fy * py) / pz + v.cy) + 0.5f);
  // (every comparison is false for NaN; a sample at or behind `near` is skipped whatever u and v came out as)
  const bool ok = pz > v.near && fu >= 0.f && fu < (float)v.W && fv >= 0.f && fv < (float)v.H;
  pix = ok ? (int)fv * v.W + (int)fu : 0;
  return ok;
}

// steps 3-5 from the pixel's values d = depth[pix], a = alpha[pix] (with_alpha) and pw = weight[pix] (or 1): false =
// skipped; otherwise the truncated distance t and the view's weight w
EGS_HD bool decide_sample(const View& v, float pz, float d, bool with_alpha, float a, float pw, float& t, float& w) {
  float zs = d;
  if (with_alpha) {
    if (!(a > v.alpha_min)) return false;
    zs = zs / a;
  }
  if (!(zs > 0.f && zs <= FLT_MAX && zs <= v.depth_max)) return false;
  const float sdf = zs - pz;
  if (!(sdf >= -v.trunc)) return false;
  t = fminf(1.f, sdf / v.trunc);
  w = pw;
  return w > 0.f && w <= FLT_MAX;
}

// steps 1-5 for one sample
EGS_HD bool sample_view(const Lattice& L, const View& v, int ix, int iy, int iz, const float* __restrict__ depth,
                        const float* __restrict__ alpha, const float* __restrict__ pixel_weight, int& pix, float& t,
                        float& w) {
  float pz;
  if (!project_sample(L, v, ix, iy, iz, pix, pz)) return false;
  return decide_sample(v, pz, depth[pix], alpha != nullptr, alpha ? alpha[pix] : 1.f,
                       pixel_weight ? pixel_weight[pix] : 1.f, t, w);
}

// step 6 for one value: the running mean `old` of weight W takes the value `val` with weight w
EGS_HD float blend(float old, float W, float val, float w) { return (W * old + w * val) / (W + w); }

// ---- marching tetrahedra ---------------------------------------------------------------------------------------------
// A corner of a cell is its offset bits dx | dy << 1 | dz << 2.  Tetrahedron k belongs to the k-th permutation (a, b, c)
// of the axes: local vertices v0 = 0, v1 = e_a, v2 = e_a + e_b, v3 = 7.  det[v1 - v0, v2 - v0, v3 - v0] = det[e_a, e_b,
// e_c] is the sign of the permutation: +, -, -, +, +, -.
//
// No case table: the triangles of a tetrahedron follow from its inside set.
//   one inside vertex i (others j < k < l): the crossings on (i,j), (i,k), (i,l).  With d_m = v_m - v_i the crossings are
//     v_i + t_m d_m, t_m > 0, and the normal n of that triangle has n . (crossing - v_i) = t_j t_k t_l det[d_j, d_k, d_l]:
//     it points away from the inside vertex iff the determinant is positive.
//   three inside (i outside): the same triangle, and the normal must point TOWARDS v_i: iff the determinant is negative.
//   two inside i < j, outside k < l: the level set of the linear interpolant is a plane, its crossings in cyclic order
//     (i,k), (i,l), (j,l), (j,k); at f_i = f_j = -1, f_k = f_l = 1 they are midpoints, the normal of the first three is
//     (v_l - v_k) x (v_j - v_i) / 4, and its product with v_k - v_i is det[d_j, d_k, d_l] / 4; the sign cannot change
//     while the inside set stays, so the quad faces outwards iff the determinant is positive.
//   det[d_j, d_k, d_l] about v_i is the tetrahedron's sign times the parity of (i, j, k, l) as a permutation of
//   (0, 1, 2, 3): odd iff i is odd (one / three inside), odd iff i + j is even (two inside).
struct Cell {
  float f[8];        // tsdf of the corners
  int64_t base;      // linear sample index of corner 0
  int cx, cy, cz;
};

EGS_HD int tet_vertex(int tet, int m) {      // corner bits of local vertex m of tetrahedron `tet`
  // the permutations (a, b, c) in lexicographic order, two bits per axis
  const int a = tet >> 1, b = (tet & 1) ? (a == 2 ? 1 : 2) : (a == 0 ? 1 : 0);
  return m == 0 ? 0 : m == 1 ? (1 << a) : m == 2 ? ((1 << a) | (1 << b)) : 7;
}
EGS_HD bool tet_negative(int tet) { return tet == 1 || tet == 2 || tet == 5; }

EGS_HD int edge_type(int d) {      // d: the offset bits of hi - lo, 1..7
  return d == 1 ? 0 : d == 2 ? 1 : d == 4 ? 2 : d == 3 ? 3 : d == 5 ? 4 : d == 6 ? 5 : 6;
}

EGS_HD int count_bits4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }

// inside mask of the 8 corners -> triangles of the cell
EGS_HD int cell_triangles(int inside8) {
  int n = 0;
  for (int tet = 0; tet < 6; ++tet) {
    int m = 0;
    for (int k = 0; k < 4; ++k) m |= ((inside8 >> tet_vertex(tet, k)) & 1) << k;
    const int c = count_bits4(m);
    n += c == 0 || c == 4 ? 0 : c == 2 ? 2 : 1;
  }
  return n;
}

// Where the corners of a cell live: key(c, p) is the linear sample index of corner p in the lattice, which names it in a
// vertex key; at(c, p) is its index in a colour plane, and `plane` the distance between two colour planes.  A dense volume
// stores a sample at its lattice index: the identity.  (A block-allocated volume, egs_sparsetsdf.hip, has its own.)
struct DenseAddr {
  int64_t sy, sz, plane;      // nx, nx ny, nx ny nz
  EGS_HD int64_t key(const Cell& c, int p) const { return c.base + (p & 1) + ((p >> 1) & 1) * sy + ((p >> 2) & 1) * sz; }
  EGS_HD int64_t at(const Cell& c, int p) const { return key(c, p); }
};

// the vertex on the edge between corners p and q of the cell (p a subset of q's bits): coordinates, key, colour
template <typename Addr, typename Out>
EGS_HD void edge_vertex(const Lattice& L, const Cell& c, int p, int q, const float* __restrict__ color, const Addr& A,
                        Out& out, int slot) {
  const int d = p ^ q;
  const float flo = c.f[p], fhi = c.f[q];
  const float t = flo / (flo - fhi);
  const float tv = t * L.voxel;
  const int lx = c.cx + (p & 1), ly = c.cy + ((p >> 1) & 1), lz = c.cz + ((p >> 2) & 1);
  const float x = (L.ox + L.voxel * (float)lx) + ((d & 1) ? tv : 0.f);
  const float y = (L.oy + L.voxel * (float)ly) + ((d & 2) ? tv : 0.f);
  const float z = (L.oz + L.voxel * (float)lz) + ((d & 4) ? tv : 0.f);
  out.vertex(slot, x, y, z, 7 * A.key(c, p) + edge_type(d));
  if (color) {
    const int64_t lo = A.at(c, p), hi = A.at(c, q);
    float rgb[3];
    for (int k = 0; k < 3; ++k) {
      const float a = color[k * A.plane + lo], b = color[k * A.plane + hi];
      rgb[k] = a + t * (b - a);
    }
    out.colour(slot, rgb[0], rgb[1], rgb[2]);
  }
}

// Emit the triangles of a cell whose corners are all valid, in order, through `out`: out.begin(k) opens the cell's k-th
// triangle (false: it has no room, the cell stops), out.vertex / out.colour fill its slots 0..2.  -> triangles emitted
template <typename Addr, typename Out>
EGS_HD int emit_cell(const Lattice& L, const Cell& c, const float* __restrict__ color, const Addr& A, Out& out) {
  int inside8 = 0;
  for (int k = 0; k < 8; ++k) inside8 |= (c.f[k] < 0.f ? 1 : 0) << k;
  int n = 0;
  for (int tet = 0; tet < 6; ++tet) {
    int v[4], m = 0;
    for (int k = 0; k < 4; ++k) {
      v[k] = tet_vertex(tet, k);
      m |= ((inside8 >> v[k]) & 1) << k;
    }
    const int cnt = count_bits4(m);
    if (cnt == 0 || cnt == 4) continue;
    const bool neg = tet_negative(tet);
    if (cnt != 2) {
      const int lone = cnt == 1 ? m : (~m & 15);      // the vertex that is alone on its side
      const int i = lone == 1 ? 0 : lone == 2 ? 1 : lone == 4 ? 2 : 3;
      const int j = i == 0 ? 1 : 0, k = i <= 1 ? 2 : 1, l = i == 3 ? 2 : 3;
      const bool positive = neg == ((i & 1) != 0);      // det[d_j, d_k, d_l] > 0
      const bool flip = cnt == 1 ? !positive : positive;
      if (!out.begin(n)) return n;
      const int e[3] = {j, flip ? l : k, flip ? k : l};
      for (int s = 0; s < 3; ++s) {
        const int a = i < e[s] ? i : e[s], b = i < e[s] ? e[s] : i;
        edge_vertex(L, c, v[a], v[b], color, A, out, s);
      }
      ++n;
    } else {
      int in[2], ou[2], ni = 0, no = 0;
      for (int k = 0; k < 4; ++k) {
        if ((m >> k) & 1) in[ni++] = k; else ou[no++] = k;
      }
      const int i = in[0], j = in[1], k = ou[0], l = ou[1];
      const bool positive = neg == (((i + j) & 1) == 0);
      // the quad (i,k), (i,l), (j,l), (j,k), or its reverse
      const int qa[4] = {i, i, j, j}, qb[4] = {k, l, l, k};
      for (int tri = 0; tri < 2; ++tri) {
        if (!out.begin(n)) return n;
        const int c1 = tri == 0 ? 1 : 2, c2 = tri == 0 ? 2 : 3;
        const int corner[3] = {0, positive ? c1 : c2, positive ? c2 : c1};
        for (int s = 0; s < 3; ++s) {
          const int p = qa[corner[s]], q = qb[corner[s]];
          edge_vertex(L, c, v[p < q ? p : q], v[p < q ? q : p], color, A, out, s);
        }
        ++n;
      }
    }
  }
  return n;
}

}  // namespace egs_tsdf
