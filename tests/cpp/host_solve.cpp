// host_solve.cpp -- TEST INFRASTRUCTURE: include/zensim_rocm/solve_device.hpp compiled for the host (g++, no HIP), under the sanitizers.
//   host_solve in.bin out.bin
// in.bin: records of 20 floats = three term blocks (elastic, barrier, friction: 6 each), scale, mass.  out.bin: per record the combined
// block (6 floats), its inverse (6 floats), the inverse applied to (1, -2, 3) (3 floats) and the fallback status (int).
// tests/test_solve_cpu.py compares the bytes with the numpy float32 replay (tests/ref64_solve.py).
#include <cstdio>
#include <vector>

#include "zensim_rocm/solve_device.hpp"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<float> rows;
  float buf[20];
  while (std::fread(buf, sizeof(float), 20, in) == 20) rows.insert(rows.end(), buf, buf + 20);
  std::fclose(in);
  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 4;
  for (size_t i = 0; i < rows.size() / 20; ++i) {
    const float *r = rows.data() + 20 * i;
    float el[6], ba[6], fr[6], D[6], inv[6], z[3];
    for (int k = 0; k < 6; ++k) el[k] = r[k], ba[k] = r[6 + k], fr[k] = r[12 + k];
    zsr::block_combine(el, ba, fr, r[18], r[19], D);
    const int status = zsr::block_inverse(D, r[19], inv);
    const float rhs[3] = {1.f, -2.f, 3.f};
    zsr::block_apply(inv, rhs, z);
    std::fwrite(D, sizeof(float), 6, out);
    std::fwrite(inv, sizeof(float), 6, out);
    std::fwrite(z, sizeof(float), 3, out);
    std::fwrite(&status, sizeof(int), 1, out);
  }
  std::fclose(out);
  return 0;
}
