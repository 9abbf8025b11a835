// host_potential.cpp -- TEST INFRASTRUCTURE: include/zensim_rocm/potential_device.hpp compiled for the host (g++, no HIP), under the
// sanitizers.
//   host_potential vertices in.bin out.bin
//       in.bin: records of 19 floats = x, target, p, start, acc (3 each), mass, scale, t, fixed (non-zero: the vertex's byte is set).
//       out.bin: per record the inertia energy, the gradient row (3), the trial position (3), the displacement (3) and whether the vertex
//       counts as fixed (int).
//   host_potential searches in.bin out.bin maxTrials
//       in.bin: records of 6 + 4 (maxTrials + 1) doubles = scale, tMax, c1, shrink, maxTrials, slope, then the four parts of E_0 and of
//       every trial.  out.bin: per record the PotentialRecord and its history of maxTrials + 1 doubles after potential_begin and
//       potential_decide on every trial while the flag is unset (zero where nothing was written).
// tests/test_potential_cpu.py compares the bytes with the numpy float32 replay (tests/ref64_potential.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zensim_rocm/potential_device.hpp"

template <class T>
static std::vector<T> read_all(const char *path) {
  std::vector<T> a;
  FILE *in = std::fopen(path, "rb");
  if (!in) return a;
  T buf[256];
  size_t n;
  while ((n = std::fread(buf, sizeof(T), 256, in)) > 0) a.insert(a.end(), buf, buf + n);
  std::fclose(in);
  return a;
}

static int vertices(const char *fin, const char *fout) {
  const std::vector<float> rows = read_all<float>(fin);
  FILE *out = std::fopen(fout, "wb");
  if (!out) return 4;
  for (size_t i = 0; i < rows.size() / 19; ++i) {
    const float *r = rows.data() + 19 * i;
    float x[3], target[3], p[3], start[3], acc[3], d[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f}, xk[3], uk[3], e = 0.f;
    for (int k = 0; k < 3; ++k) x[k] = r[k], target[k] = r[3 + k], p[k] = r[6 + k], start[k] = r[9 + k], acc[k] = r[12 + k];
    const float mass = r[15], scale = r[16], t = r[17];
    const unsigned char byte = r[18] != 0.f;
    const int fixed = zsr::potential_fixed(&mass, &byte, 0);
    if (!fixed) {
      e = zsr::potential_inertia(x, target, mass, d);
      zsr::potential_gradient(mass, d, scale, acc, g);
    }
    zsr::potential_trial(x, p, t, fixed != 0, xk);
    zsr::potential_displacement(xk, start, uk);
    std::fwrite(&e, sizeof(float), 1, out);
    std::fwrite(g, sizeof(float), 3, out);
    std::fwrite(xk, sizeof(float), 3, out);
    std::fwrite(uk, sizeof(float), 3, out);
    std::fwrite(&fixed, sizeof(int), 1, out);
  }
  std::fclose(out);
  return 0;
}

static int searches(const char *fin, const char *fout, int maxTrials) {
  const std::vector<double> rows = read_all<double>(fin);
  const size_t width = 6 + 4 * ((size_t)maxTrials + 1);
  FILE *out = std::fopen(fout, "wb");
  if (!out) return 4;
  for (size_t i = 0; i < rows.size() / width; ++i) {
    const double *r = rows.data() + width * i;
    const float scale = (float)r[0], tMax = (float)r[1], c1 = (float)r[2], shrink = (float)r[3];
    const double slope = r[5];
    const auto energy = [&](int k) {
      const double parts[4] = {r[6 + 4 * k], r[7 + 4 * k], r[8 + 4 * k], r[9 + 4 * k]};
      return zsr::potential_energy(parts, scale);
    };
    zsr::PotentialRecord rec;
    std::memset(&rec, 0, sizeof(rec));
    std::vector<double> history((size_t)maxTrials + 1, 0.0);
    zsr::potential_begin(rec, history.data(), energy(0), slope, tMax);
    for (int k = 1; k <= maxTrials && rec.flag == zsr::POTENTIAL_RUNNING; ++k)
      zsr::potential_decide(rec, history.data(), energy(k), c1, shrink, maxTrials);
    std::fwrite(&rec, sizeof(rec), 1, out);
    std::fwrite(history.data(), sizeof(double), history.size(), out);
  }
  std::fclose(out);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !std::strcmp(argv[1], "vertices")) return vertices(argv[2], argv[3]);
  if (argc == 5 && !std::strcmp(argv[1], "searches")) return searches(argv[2], argv[3], std::atoi(argv[4]));
  return 2;
}
