// Keyframed level-set colliders through the C++ face: two SparseGrid<3, f32, 8> keyframes of a sphere that moves by 1.5 cells ("sdf" and a
// uniform material velocity "v"), blended by TransitionLevelSetView{viewA, viewB, stepDt, alpha} in a user lambda -- the three level-set
// calls against zs_rocm_levelset_transition_sample, and Collider{transition, type}.resolveCollision(x, v) for the three collider types
// with the identity and with a moving transform against zs_rocm_levelset_transition_collider_resolve, bit for bit.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include tests/cpp/test_transition.hip -L zpc_amd/lib -lzsrocm
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  const float h = 1.f / 32, band = 0.2f, radius = 0.3f;
  const float stepDt = 0.01f, alpha = 0.25f;
  const float shift[3] = {1.5f * h * 0.6f, 1.5f * h * -0.48f, 1.5f * h * 0.64f};
  SparseGrid<3, float, 8> grids[2] = {SparseGrid<3, float, 8>(std::vector<PropertyTag>{{"sdf", 1}, {"v", 3}}, 2048),
                                      SparseGrid<3, float, 8>(std::vector<PropertyTag>{{"sdf", 1}, {"v", 3}}, 2048)};
  for (int k = 0; k < 2; ++k) {
  SparseGrid<3, float, 8> &sg = grids[k];
  const float c0 = 0.5f + k * shift[0], c1 = 0.47f + k * shift[1], c2 = 0.53f + k * shift[2];
  const float u0 = shift[0] / stepDt, u1 = shift[1] / stepDt, u2 = shift[2] / stepDt;
  sg.scale(h);
  sg._background = band;
  // blocks around the surface: a lattice of spacing 4 cells, every point within the band inserts its block
  const int nl = 33 * 2;
  pol(range((long long)nl * nl * nl), [g = view<space>(sg), nl, h, band, radius, c0, c1, c2] ZS_LAMBDA(long long i) {
    const V3 p{{(float)(i / (nl * nl)) * 4 * h - 1.f, (float)(i / nl % nl) * 4 * h - 1.f, (float)(i % nl) * 4 * h - 1.f}};
    const float d = sqrtf((p[0] - c0) * (p[0] - c0) + (p[1] - c1) * (p[1] - c1) + (p[2] - c2) * (p[2] - c2)) - radius;
    if (fabsf(d) < band) g.insert(p);
  });
  const std::size_t nb = sg.numBlocks();
  CHECK(nb > 20 && nb < 2000);
  pol(range((long long)nb * 512), [g = view<space>(sg), radius, c0, c1, c2, u0, u1, u2] ZS_LAMBDA(long long c) {
    const int b = (int)(c / 512), k = (int)(c % 512);
    const auto w = g.wCoord(b, k);
    g("sdf", 0, b, k) = sqrtf((w[0] - c0) * (w[0] - c0) + (w[1] - c1) * (w[1] - c1) + (w[2] - c2) * (w[2] - c2)) - radius;
    g("v", 0, b, k) = u0 + 0.3f * w[1];
    g("v", 1, b, k) = u1 - 0.2f * w[2];
    g("v", 2, b, k) = u2 + 0.25f * w[0];
  });
  }
  const int np = 40000;
  Vector<float> px(3 * np, memsrc_e::um), v0(3 * np, memsrc_e::um), va(3 * np, memsrc_e::um), vb(3 * np, memsrc_e::um);
  Vector<int> ia(np, memsrc_e::um), ib(np, memsrc_e::um);
  unsigned s = 7u;
  for (int i = 0; i < 3 * np; ++i) {
    s = s * 1664525u + 1013904223u;
    px.data()[i] = 0.1f + 0.8f * (float)(s >> 8) / (float)(1u << 24);
    s = s * 1664525u + 1013904223u;
    v0.data()[i] = -1.f + 2.f * (float)(s >> 8) / (float)(1u << 24);
  }
  TransitionLevelSetView gv{view<space>(grids[0]), view<space>(grids[1]), stepDt, alpha};
  zs_rocm_levelset_transition ls{};
  ls.src = gv.src.levelSetView();
  ls.dst = gv.dst.levelSetView();
  ls.stepDt = stepDt;
  ls.alpha = alpha;
  ls.maxSpeed = 3.f;
  CHECK(ls.src.velChannel == 1 && ls.dst.velChannel == 1 && ls.src.tiles != ls.dst.tiles);
  // the three level-set calls of the transition against the bulk sampling entry
  {
    Vector<float> sa(7 * np, memsrc_e::um), sb(7 * np, memsrc_e::um);
    pol(range(np), [g = gv, p = view<space>(px), o = view<space>(sa)] ZS_LAMBDA(long long i) {
      const V3 x{{p[3 * i], p[3 * i + 1], p[3 * i + 2]}};
      o[7 * i] = g.getSignedDistance(x);
      const V3 n = g.getNormal(x), vm = g.getMaterialVelocity(x);
      for (int d = 0; d < 3; ++d) { o[7 * i + 1 + d] = n[d]; o[7 * i + 4 + d] = vm[d]; }
    });
    Vector<float> sd(np, memsrc_e::um), nn(3 * np, memsrc_e::um), vm(3 * np, memsrc_e::um);
    CHECK(zs_rocm_levelset_transition_sample(pol.handle(), &ls, px.data(), np, sd.data(), nn.data(), vm.data()) == 0);
    zs_rocm_policy_sync_ctx(pol.handle());
    int bad = 0, negative = 0;
    for (int i = 0; i < np; ++i) {
      bad += std::memcmp(&sa.data()[7 * i], &sd.data()[i], 4) != 0;
      bad += std::memcmp(&sa.data()[7 * i + 1], &nn.data()[3 * i], 12) != 0;
      bad += std::memcmp(&sa.data()[7 * i + 4], &vm.data()[3 * i], 12) != 0;
      negative += sd.data()[i] < 0.f;
    }
    std::printf("transition sample: %d points, %d inside, %d mismatches\n", np, negative, bad);
    CHECK(bad == 0 && negative > 1000);
  }
  int total = 0;
  for (int moving = 0; moving < 2; ++moving)
    for (int type = 0; type < 3; ++type) {
      Collider col{gv, (collider_e)type};
      if (moving) {
        const float a = 0.3f, ca = cosf(a), sa = sinf(a);
        const float R[9] = {ca, -sa, 0.f, sa, ca, 0.f, 0.f, 0.f, 1.f};
        for (int i = 0; i < 9; ++i) col.R[i] = R[i];
        col.s = 1.1f;
        col.dsdt = 0.2f;
        col.omega[0] = 0.1f; col.omega[1] = -0.3f; col.omega[2] = 0.2f;
        col.b[0] = 0.05f; col.b[1] = -0.08f; col.b[2] = 0.03f;
        col.dbdt[0] = 0.4f; col.dbdt[1] = 0.1f; col.dbdt[2] = -0.2f;
      }
      std::memcpy(va.data(), v0.data(), sizeof(float) * 3 * np);
      std::memcpy(vb.data(), v0.data(), sizeof(float) * 3 * np);
      pol(range(np), [col, p = view<space>(px), v = view<space>(va), in = view<space>(ia)] ZS_LAMBDA(long long i) {
        const V3 x{{p[3 * i], p[3 * i + 1], p[3 * i + 2]}};
        V3 u{{v[3 * i], v[3 * i + 1], v[3 * i + 2]}};
        const bool inside = col.resolveCollision(x, u);
        if (inside)
          for (int d = 0; d < 3; ++d) v[3 * i + d] = u[d];
        in[i] = inside ? 1 : 0;
        if (inside != col.queryInside(x)) in[i] = -1;
      });
      zs_rocm_collider c{};
      zs_rocm_collider_init(&c, ZS_ROCM_GEOM_PLANE, type, nullptr, 0);
      c.s = col.s;
      c.dsdt = col.dsdt;
      for (int i = 0; i < 9; ++i) c.R[i] = col.R[i];
      for (int i = 0; i < 3; ++i) { c.omega[i] = col.omega[i]; c.b[i] = col.b[i]; c.dbdt[i] = col.dbdt[i]; }
      CHECK(zs_rocm_levelset_transition_collider_resolve(pol.handle(), &c, &ls, px.data(), vb.data(), np, ib.data()) == 0);
      zs_rocm_policy_sync_ctx(pol.handle());
      int bad = 0, inside = 0, changed = 0;
      for (int i = 0; i < np; ++i) {
        bad += ia.data()[i] != ib.data()[i];
        bad += std::memcmp(&va.data()[3 * i], &vb.data()[3 * i], 12) != 0;
        inside += ib.data()[i];
        changed += std::memcmp(&va.data()[3 * i], &v0.data()[3 * i], 12) != 0;
      }
      std::printf("transition collider: type %d moving %d: %d inside, %d changed, %d mismatches\n", type, moving, inside, changed, bad);
      CHECK(bad == 0 && inside > 1000 && changed > 1000 && changed <= inside);
      total += bad;
    }
  // argument checks of the C entry: refused with nothing written
  {
    zs_rocm_collider c{};
    zs_rocm_collider_init(&c, ZS_ROCM_GEOM_PLANE, ZS_ROCM_COLLIDER_SLIP, nullptr, 0);
    zs_rocm_levelset_transition badls = ls;
    badls.alpha = 1.5f;
    std::memcpy(vb.data(), v0.data(), sizeof(float) * 3 * np);
    CHECK(zs_rocm_levelset_transition_collider_resolve(pol.handle(), &c, &badls, px.data(), vb.data(), np, nullptr) == -1);
    c.type = 3;
    CHECK(zs_rocm_levelset_transition_collider_resolve(pol.handle(), &c, &ls, px.data(), vb.data(), np, nullptr) == -1);
    zs_rocm_policy_sync_ctx(pol.handle());
    CHECK(std::memcmp(vb.data(), v0.data(), sizeof(float) * 3 * np) == 0);
  }
  std::printf("transition cpp face ok: %d mismatches\n", total);
  return 0;
}
