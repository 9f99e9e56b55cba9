// A host program around csrc/egs_tsdf_device.h, compiled by tests/test_sparse_tsdf_cpu.py with a plain C++ compiler: one
// view into dense planes through sample_view / blend, then the cells through emit_cell with the dense addressing.  What
// the dense kernels do, without a GPU: it shows that the functions both volumes share still compute the reference.
//
//   tsdf_host_check IN OUT
//   IN : int32 nx ny nz H W has_alpha has_weight has_color; float32 ox oy oz voxel fx fy cx cy R[9] t[3] trunc alpha_min near
//        depth_max min_weight; depth [H W], alpha, weight, image [3 H W] (those present); tsdf [N], weight [N], color [3 N]
//   OUT: tsdf, weight, color; int64 T; verts [T 9] float32, keys [T 3] int64, colors [T 9] float32 (with colour)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../easygaussiansplatting_amd/csrc/egs_tsdf_device.h"

struct Soup {
  std::vector<float> verts, colors;
  std::vector<int64_t> keys;
  int64_t first = 0, tri = 0;
  bool begin(int k) {
    tri = first + k;
    verts.resize((tri + 1) * 9);
    keys.resize((tri + 1) * 3);
    colors.resize((tri + 1) * 9);
    return true;
  }
  void vertex(int slot, float x, float y, float z, int64_t key) {
    float* p = &verts[(tri * 3 + slot) * 3];
    p[0] = x; p[1] = y; p[2] = z;
    keys[tri * 3 + slot] = key;
  }
  void colour(int slot, float r, float g, float b) {
    float* p = &colors[(tri * 3 + slot) * 3];
    p[0] = r; p[1] = g; p[2] = b;
  }
};

template <typename T>
static std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
template <typename T>
static void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const auto hd = take<int32_t>(in, 8);
  const auto fl = take<float>(in, 25);
  egs_tsdf::Lattice L = {hd[0], hd[1], hd[2], fl[0], fl[1], fl[2], fl[3]};
  egs_tsdf::View v;
  v.H = hd[3]; v.W = hd[4];
  v.fx = fl[4]; v.fy = fl[5]; v.cx = fl[6]; v.cy = fl[7];
  for (int k = 0; k < 9; ++k) v.R[k] = fl[8 + k];
  for (int k = 0; k < 3; ++k) v.t[k] = fl[17 + k];
  v.trunc = fl[20]; v.alpha_min = fl[21]; v.near = fl[22]; v.depth_max = fl[23];
  const float min_weight = fl[24];
  const size_t npix = (size_t)v.H * v.W, N = (size_t)L.nx * L.ny * L.nz;
  const auto depth = take<float>(in, npix);
  const auto alpha = take<float>(in, hd[5] ? npix : 0), pw = take<float>(in, hd[6] ? npix : 0);
  const auto image = take<float>(in, hd[7] ? 3 * npix : 0);
  auto tsdf = take<float>(in, N), weight = take<float>(in, N);
  auto color = take<float>(in, hd[7] ? 3 * N : 0);
  fclose(in);

  for (int iz = 0; iz < L.nz; ++iz)
    for (int iy = 0; iy < L.ny; ++iy)
      for (int ix = 0; ix < L.nx; ++ix) {
        int pix;
        float t, w;
        if (!egs_tsdf::sample_view(L, v, ix, iy, iz, depth.data(), hd[5] ? alpha.data() : nullptr,
                                   hd[6] ? pw.data() : nullptr, pix, t, w))
          continue;
        const size_t i = ((size_t)iz * L.ny + iy) * L.nx + ix;
        const float W0 = weight[i];
        tsdf[i] = egs_tsdf::blend(tsdf[i], W0, t, w);
        for (int c = 0; c < (hd[7] ? 3 : 0); ++c) color[c * N + i] = egs_tsdf::blend(color[c * N + i], W0, image[c * npix + pix], w);
        weight[i] = W0 + w;
      }

  Soup out;
  const egs_tsdf::DenseAddr addr = {L.nx, (int64_t)L.nx * L.ny, (int64_t)N};
  for (int cz = 0; cz + 1 < L.nz; ++cz)
    for (int cy = 0; cy + 1 < L.ny; ++cy)
      for (int cx = 0; cx + 1 < L.nx; ++cx) {
        egs_tsdf::Cell c;
        c.cx = cx; c.cy = cy; c.cz = cz;
        c.base = ((int64_t)cz * L.ny + cy) * L.nx + cx;
        bool valid = true;
        for (int k = 0; k < 8; ++k) {
          const int64_t i = addr.key(c, k);
          valid = valid && weight[i] >= min_weight;
          c.f[k] = tsdf[i];
        }
        if (valid) out.first += egs_tsdf::emit_cell(L, c, hd[7] ? color.data() : nullptr, addr, out);
      }

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  put(o, tsdf); put(o, weight); put(o, color);
  const int64_t T = out.first;
  fwrite(&T, sizeof(T), 1, o);
  out.verts.resize(T * 9); out.keys.resize(T * 3); out.colors.resize(hd[7] ? T * 9 : 0);
  put(o, out.verts); put(o, out.keys); put(o, out.colors);
  fclose(o);
  return 0;
}
