// Triangle-mesh colliders through the C++ face: a user lambda calls TriMeshView::signed_distance(p) and closest_point(p) on an
// octahedron-based sphere mesh, and the results equal zs_rocm_mesh_signed_distance / zs_rocm_mesh_closest_point of the C ABI on the same
// points bit for bit.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include tests/cpp/test_mesh.hip -L zpc_amd/lib -lzsrocm
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "zensim_rocm/zs_rocm.hpp"

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                              \
    }                                                            \
  } while (0)

using namespace zs;
constexpr auto space = execspace_e::rocm;
using V3 = small_vec<float, 3>;

int main() {
  auto pol = rocm_exec();
  // an octahedron subdivided four times and pushed onto the sphere of radius 0.3 around (0.5, 0.47, 0.53): 2048 triangles, outward
  std::vector<float> v = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
  std::vector<int> t = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
  for (int level = 0; level < 4; ++level) {
    std::map<std::pair<int, int>, int> mid;
    auto m = [&](int i, int j) {
      const auto k = std::make_pair(i < j ? i : j, i < j ? j : i);
      auto it = mid.find(k);
      if (it != mid.end()) return it->second;
      float x[3], l = 0.f;
      for (int d = 0; d < 3; ++d) { x[d] = v[3 * i + d] + v[3 * j + d]; l += x[d] * x[d]; }
      for (int d = 0; d < 3; ++d) v.push_back(x[d] / std::sqrt(l));
      return mid[k] = (int)v.size() / 3 - 1;
    };
    std::vector<int> nt;
    for (std::size_t f = 0; f < t.size(); f += 3) {
      const int a = t[f], b = t[f + 1], c = t[f + 2], ab = m(a, b), bc = m(b, c), ca = m(c, a);
      const int add[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
      nt.insert(nt.end(), add, add + 12);
    }
    t.swap(nt);
  }
  const float centre[3] = {0.5f, 0.47f, 0.53f};
  const int nv = (int)v.size() / 3, ntri = (int)t.size() / 3;
  Vector<float> verts(3 * nv, memsrc_e::um), vel(3 * nv, memsrc_e::um);
  Vector<int> tris(3 * ntri, memsrc_e::um);
  for (int i = 0; i < 3 * nv; ++i) {
    verts.data()[i] = centre[i % 3] + 0.3f * v[i];
    vel.data()[i] = 0.25f * v[i] + 0.1f * (float)(i % 3);
  }
  std::memcpy(tris.data(), t.data(), sizeof(int) * t.size());
  TriMesh mesh(pol, verts, tris, &vel);
  zs_rocm_policy_sync_ctx(pol.handle());
  int st[ZS_ROCM_MESH_STAT_WORDS];
  zs_rocm_mesh_stats(pol.handle(), mesh.handle(), st);
  CHECK(ntri == 2048 && st[0] == 0 && st[1] == 0 && st[2] == 0 && st[3] == 0 && st[4] == 0);

  const int np = 40000;
  Vector<float> px(3 * np, memsrc_e::um), sa(np, memsrc_e::um), sb(np, memsrc_e::um), da(np, memsrc_e::um), db(np, memsrc_e::um);
  Vector<float> va(3 * np, memsrc_e::um), vb(3 * np, memsrc_e::um), ba(3 * np, memsrc_e::um), bb(3 * np, memsrc_e::um);
  Vector<int> ta(np, memsrc_e::um), tb(np, memsrc_e::um), fa(np, memsrc_e::um), fb(np, memsrc_e::um);
  unsigned s = 11u;
  for (int i = 0; i < 3 * np; ++i) {
    s = s * 1664525u + 1013904223u;
    px.data()[i] = (float)(s >> 8) / (float)(1u << 24);
  }
  pol(range(np), [m = view<space>(mesh), p = view<space>(px), sd = view<space>(sa), dd = view<space>(da), vv = view<space>(va),
                  bw = view<space>(ba), tt = view<space>(ta), ff = view<space>(fa)] ZS_LAMBDA(long long i) {
    const V3 x{{p[3 * i], p[3 * i + 1], p[3 * i + 2]}};
    sd[i] = m.signed_distance(x);
    const auto c = m.closest_point(x);
    const V3 u = m.velocity(c);
    dd[i] = c.dist;
    tt[i] = c.tri;
    ff[i] = c.feature;
    for (int d = 0; d < 3; ++d) { vv[3 * i + d] = u[d]; bw[3 * i + d] = c.bary[d]; }
  });
  CHECK(zs_rocm_mesh_signed_distance(pol.handle(), mesh.handle(), px.data(), np, 3.402823466e+38f, sb.data(), vb.data()) == 0);
  CHECK(zs_rocm_mesh_closest_point(pol.handle(), mesh.handle(), px.data(), np, 3.402823466e+38f, db.data(), tb.data(), fb.data(), bb.data()) == 0);
  zs_rocm_policy_sync_ctx(pol.handle());
  int bad = 0, inside = 0, wrongSign = 0;
  for (int i = 0; i < np; ++i) {
    bad += std::memcmp(&sa.data()[i], &sb.data()[i], 4) != 0;
    bad += std::memcmp(&da.data()[i], &db.data()[i], 4) != 0;
    bad += std::memcmp(&va.data()[3 * i], &vb.data()[3 * i], 12) != 0;
    bad += std::memcmp(&ba.data()[3 * i], &bb.data()[3 * i], 12) != 0;
    bad += ta.data()[i] != tb.data()[i] || fa.data()[i] != fb.data()[i];
    inside += sb.data()[i] < 0.f;
    const float *x = &px.data()[3 * i];
    const float r = std::sqrt((x[0] - centre[0]) * (x[0] - centre[0]) + (x[1] - centre[1]) * (x[1] - centre[1]) + (x[2] - centre[2]) * (x[2] - centre[2]));
    if (std::fabs(r - 0.3f) > 0.01f) wrongSign += (r < 0.3f) != (sb.data()[i] < 0.f);  // (the mesh lies within 0.002 of the sphere)
  }
  std::printf("mesh cpp face: %d points, %d inside, %d mismatches, %d wrong signs\n", np, inside, bad, wrongSign);
  CHECK(bad == 0 && wrongSign == 0 && inside > 2000);
  // argument checks of the C entries: refused with nothing written
  CHECK(zs_rocm_mesh_signed_distance(pol.handle(), nullptr, px.data(), np, 1.f, sb.data(), nullptr) == -1);
  CHECK(zs_rocm_mesh_closest_point(pol.handle(), mesh.handle(), nullptr, np, 1.f, db.data(), nullptr, nullptr, nullptr) == -1);
  std::printf("mesh cpp face ok\n");
  return 0;
}
