// host_ee_closest.cpp -- zsr::ee_closest (include/zensim_rocm/distance_device.hpp) on the host: reads n segment pairs (12 floats each: a0, a1,
// b0, b1) from the binary file argv[1] and writes per pair dist2, s, t (floats) and the category (int) to argv[2].  Built by
// tests/test_proximity_cpu.py with the host compiler, without FP contraction and under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <vector>

#include "zensim_rocm/distance_device.hpp"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<float> buf;
  float rec[12];
  while (std::fread(rec, sizeof(float), 12, in) == 12) buf.insert(buf.end(), rec, rec + 12);
  std::fclose(in);
  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 4;
  const size_t n = buf.size() / 12;
  for (size_t i = 0; i < n; ++i) {
    const float *p = buf.data() + 12 * i;
    const float a0[3] = {p[0], p[1], p[2]}, a1[3] = {p[3], p[4], p[5]}, b0[3] = {p[6], p[7], p[8]}, b1[3] = {p[9], p[10], p[11]};
    const zsr::EdgeClosest r = zsr::ee_closest(a0, a1, b0, b1);
    const float f[3] = {r.dist2, r.s, r.t};
    std::fwrite(f, sizeof(float), 3, out);
    std::fwrite(&r.category, sizeof(int), 1, out);
  }
  std::fclose(out);
  std::printf("%zu pairs\n", n);
  return 0;
}
