// host_friction.cpp -- zsr::friction_lag_pt / _ee and friction_energy / _gradient / _product (include/zensim_rocm/friction_device.hpp) on the
// host: reads n records of 44 floats from the binary file argv[1] (four points, then dHat2, kappa, the mollifier threshold eps, one unused;
// the rows u[4][3] and x[4][3] of the four corners; mu, eps_v, two unused) and writes per record to argv[2]: the lag record (8 floats) and
// its status (int); the energy of the energy call and its status; the energy, the gradient [4][3] and the status of the gradient call; the
// product [4][3] and its status.  argv[3] = "pt" or "ee".  Built by tests/test_friction_cpu.py with the host compiler, without FP
// contraction and under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "zensim_rocm/friction_device.hpp"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const bool pt = std::strcmp(argv[3], "pt") == 0;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  constexpr int W = 44;
  std::vector<float> buf;
  float rec[W];
  while (std::fread(rec, sizeof(float), W, in) == W) buf.insert(buf.end(), rec, rec + W);
  std::fclose(in);
  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 4;
  const size_t n = buf.size() / W;
  for (size_t i = 0; i < n; ++i) {
    const float *p = buf.data() + W * i;
    const float x0[3] = {p[0], p[1], p[2]}, x1[3] = {p[3], p[4], p[5]}, x2[3] = {p[6], p[7], p[8]}, x3[3] = {p[9], p[10], p[11]};
    float u[4][3], x[4][3];
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < 3; ++d) u[k][d] = p[16 + 3 * k + d], x[k][d] = p[28 + 3 * k + d];
    const float mu = p[40], epsv = p[41];
    zsr::FrictionRecord r;
    const int lag = pt ? zsr::friction_lag_pt(x0, x1, x2, x3, p[12], p[13], r) : zsr::friction_lag_ee(x0, x1, x2, x3, p[12], p[13], p[14], r);
    float e, eg, g[4][3], h[4][3];
    const int se = zsr::friction_energy(r, u, mu, epsv, e);
    const int sg = zsr::friction_gradient(r, u, mu, epsv, eg, g);
    const int sh = zsr::friction_product(r, u, x, mu, epsv, h);
    std::fwrite(r.n, sizeof(float), 3, out);
    std::fwrite(&r.lambda, sizeof(float), 1, out);
    std::fwrite(r.w, sizeof(float), 4, out);
    std::fwrite(&lag, sizeof(int), 1, out);
    std::fwrite(&e, sizeof(float), 1, out);
    std::fwrite(&se, sizeof(int), 1, out);
    std::fwrite(&eg, sizeof(float), 1, out);
    std::fwrite(g, sizeof(float), 12, out);
    std::fwrite(&sg, sizeof(int), 1, out);
    std::fwrite(h, sizeof(float), 12, out);
    std::fwrite(&sh, sizeof(int), 1, out);
  }
  std::fclose(out);
  std::printf("%zu pairs\n", n);
  return 0;
}
