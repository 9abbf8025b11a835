// host_elastic.cpp -- the membrane and bending functions of include/zensim_rocm/elastic_device.hpp on the host: reads n records of 40 floats
// from the binary file argv[1] (four rest points, four points x, four direction rows z -- a triangle uses the first three of each -- then
// mu, lam, kb, one unused) and writes per record to argv[2]: the rest record (4 floats) and its status (int); the energy of the energy call
// and its status; the energy, the gradient [4][3] and the status of the gradient call; the product [4][3] and its status; the psd product
// [4][3] and its status (a hinge: the same product again).  argv[3] = "tri" or "hinge"; a triangle's fourth rows are written as zeros.  Built by
// tests/test_elastic_cpu.py with the host compiler, without FP contraction and under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "zensim_rocm/elastic_device.hpp"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const bool tri = std::strcmp(argv[3], "tri") == 0;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  constexpr int W = 40;
  std::vector<float> buf;
  float row[W];
  while (std::fread(row, sizeof(float), W, in) == W) buf.insert(buf.end(), row, row + W);
  std::fclose(in);
  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 4;
  const size_t n = buf.size() / W;
  for (size_t i = 0; i < n; ++i) {
    const float *p = buf.data() + W * i;
    float X[4][3], x[4][3], z[4][3];
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < 3; ++d) X[k][d] = p[3 * k + d], x[k][d] = p[12 + 3 * k + d], z[k][d] = p[24 + 3 * k + d];
    const float mu = p[36], lam = p[37], kb = p[38];
    float rec[4], e = 0.f, eg = 0.f, g[4][3] = {}, h[4][3] = {}, hp[4][3] = {};
    int sr, se, sg, sh, sp;
    if (tri) {
      float x3[3][3], z3[3][3], g3[3][3], h3[3][3], hp3[3][3];
      std::memcpy(x3, x, sizeof(x3));
      std::memcpy(z3, z, sizeof(z3));
      sr = zsr::elastic_tri_rest(X[0], X[1], X[2], rec);
      se = zsr::elastic_tri_energy(rec, x3, mu, lam, e);
      sg = zsr::elastic_tri_gradient(rec, x3, mu, lam, eg, g3);
      sh = zsr::elastic_tri_product<false>(rec, x3, z3, mu, lam, h3);
      sp = zsr::elastic_tri_product<true>(rec, x3, z3, mu, lam, hp3);
      std::memcpy(g, g3, sizeof(g3));
      std::memcpy(h, h3, sizeof(h3));
      std::memcpy(hp, hp3, sizeof(hp3));
    } else {
      sr = zsr::elastic_hinge_rest(X[0], X[1], X[2], X[3], rec);
      se = zsr::elastic_hinge_energy(rec, x, kb, e);
      sg = zsr::elastic_hinge_gradient(rec, x, kb, eg, g);
      sh = zsr::elastic_hinge_product(rec, z, kb, h);
      sp = zsr::elastic_hinge_product(rec, z, kb, hp);
    }
    std::fwrite(rec, sizeof(float), 4, out);
    std::fwrite(&sr, sizeof(int), 1, out);
    std::fwrite(&e, sizeof(float), 1, out);
    std::fwrite(&se, sizeof(int), 1, out);
    std::fwrite(&eg, sizeof(float), 1, out);
    std::fwrite(g, sizeof(float), 12, out);
    std::fwrite(&sg, sizeof(int), 1, out);
    std::fwrite(h, sizeof(float), 12, out);
    std::fwrite(&sh, sizeof(int), 1, out);
    std::fwrite(hp, sizeof(float), 12, out);
    std::fwrite(&sp, sizeof(int), 1, out);
  }
  std::fclose(out);
  std::printf("%zu elements\n", n);
  return 0;
}
