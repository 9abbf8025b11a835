// host_barrier_hessian.cpp -- zsr::barrier_pt_hvp / barrier_ee_hvp (include/zensim_rocm/barrier_device.hpp) on the host: reads n records of 28
// floats from the binary file argv[1] (four points, then dHat2, kappa, the mollifier threshold eps, psd as 0 or 1, then the four rows of the
// direction) and writes per record the product [4][3] (floats) and the status (int) to argv[2]; argv[3] = "pt" or "ee".  Built by
// tests/test_barrier_hessian_cpu.py with the host compiler, without FP contraction and under the address and undefined-behaviour sanitizers.
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
  float rec[28];
  while (std::fread(rec, sizeof(float), 28, in) == 28) buf.insert(buf.end(), rec, rec + 28);
  std::fclose(in);
  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 4;
  const size_t n = buf.size() / 28;
  for (size_t i = 0; i < n; ++i) {
    const float *p = buf.data() + 28 * i;
    const float x0[3] = {p[0], p[1], p[2]}, x1[3] = {p[3], p[4], p[5]}, x2[3] = {p[6], p[7], p[8]}, x3[3] = {p[9], p[10], p[11]};
    float dir[4][3], h[4][3];
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < 3; ++d) dir[k][d] = p[16 + 3 * k + d];
    const bool psd = p[15] != 0.f;
    int status;
    if (pt)
      status = psd ? zsr::barrier_pt_hvp<true>(x0, x1, x2, x3, dir, p[12], p[13], h) : zsr::barrier_pt_hvp<false>(x0, x1, x2, x3, dir, p[12], p[13], h);
    else
      status = psd ? zsr::barrier_ee_hvp<true>(x0, x1, x2, x3, dir, p[12], p[13], p[14], h)
                   : zsr::barrier_ee_hvp<false>(x0, x1, x2, x3, dir, p[12], p[13], p[14], h);
    std::fwrite(h, sizeof(float), 12, out);
    std::fwrite(&status, sizeof(int), 1, out);
  }
  std::fclose(out);
  std::printf("%zu pairs\n", n);
  return 0;
}
