// host_barrier.cpp -- zsr::barrier_pt / barrier_ee (include/zensim_rocm/barrier_device.hpp) on the host: reads n records of 16 floats from the
// binary file argv[1] (four points, then dHat2, kappa, the mollifier threshold eps, one unused) and writes per record the energy, the
// gradient [4][3] (floats) and the status (int) to argv[2]; argv[3] = "pt" or "ee".  Built by tests/test_barrier_cpu.py with the host
// compiler, without FP contraction and under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "zensim_rocm/barrier_device.hpp"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const bool pt = std::strcmp(argv[3], "pt") == 0;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<float> buf;
  float rec[16];
  while (std::fread(rec, sizeof(float), 16, in) == 16) buf.insert(buf.end(), rec, rec + 16);
  std::fclose(in);
  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 4;
  const size_t n = buf.size() / 16;
  for (size_t i = 0; i < n; ++i) {
    const float *p = buf.data() + 16 * i;
    const float x0[3] = {p[0], p[1], p[2]}, x1[3] = {p[3], p[4], p[5]}, x2[3] = {p[6], p[7], p[8]}, x3[3] = {p[9], p[10], p[11]};
    float e, g[4][3];
    const int status = pt ? zsr::barrier_pt<true>(x0, x1, x2, x3, p[12], p[13], e, g) : zsr::barrier_ee<true>(x0, x1, x2, x3, p[12], p[13], p[14], e, g);
    std::fwrite(&e, sizeof(float), 1, out);
    std::fwrite(g, sizeof(float), 12, out);
    std::fwrite(&status, sizeof(int), 1, out);
  }
  std::fclose(out);
  std::printf("%zu pairs\n", n);
  return 0;
}
