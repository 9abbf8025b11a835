// host_ccd.cpp -- zsr::ccd_pt / ccd_ee (include/zensim_rocm/ccd_device.hpp) on the host: reads records of 28 floats from stdin (the four
// positions, the four direction rows, then slack, tMax, maxIter as a float, one unused) and writes per record t (float), the status and the
// number of distance evaluations (ints) to stdout; argv[1] = "pt" or "ee".  Built by tests/test_ccd_cpu.py with the host compiler, without
// FP contraction and under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "zensim_rocm/ccd_device.hpp"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const bool pt = std::strcmp(argv[1], "pt") == 0;
  std::vector<float> buf;
  float rec[28];
  while (std::fread(rec, sizeof(float), 28, stdin) == 28) buf.insert(buf.end(), rec, rec + 28);
  const size_t n = buf.size() / 28;
  for (size_t i = 0; i < n; ++i) {
    const float *r = buf.data() + 28 * i;
    float x[4][3], p[4][3];
    std::memcpy(x, r, sizeof(x));
    std::memcpy(p, r + 12, sizeof(p));
    int status = 0, evals = 0;
    const float t = pt ? zsr::ccd_pt(x, p, r[24], r[25], (int)r[26], status, &evals) : zsr::ccd_ee(x, p, r[24], r[25], (int)r[26], status, &evals);
    std::fwrite(&t, sizeof(float), 1, stdout);
    std::fwrite(&status, sizeof(int), 1, stdout);
    std::fwrite(&evals, sizeof(int), 1, stdout);
  }
  std::fflush(stdout);
  std::fprintf(stderr, "%zu pairs\n", n);
  return 0;
}
