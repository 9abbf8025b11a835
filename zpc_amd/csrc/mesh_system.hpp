// mesh_system.hpp -- what mesh_solve.hip (the Newton system) and mesh_potential.hip (the incremental potential) share on the host around the
// descriptor zs_rocm_mesh_system: where the terms of the three element-kernel families sit in one scratch array, and the argument checks.
#pragma once
#include <cfloat>

#include "mesh_pairs.hpp"

namespace zsr {

// where the terms of the three products sit in the scratch array (floats per corner: 3 for the operator, 6 for the blocks)
struct SystemLayout {
  size_t elastic, barrier, friction, total;
};
inline SystemLayout system_layout(const zs_rocm_mesh *m, const zs_rocm_mesh_system &s, size_t perCorner) {
  SystemLayout l;
  const auto pad = [](size_t n) { return (n + 63) & ~(size_t)63; };  // every part starts 256-byte aligned (the pair kernels store float4)
  l.elastic = 0;
  l.barrier = s.elastic ? pad(perCorner * (3 * m->nt + 4 * m->nh)) : 0;
  l.friction = l.barrier + (s.barrier ? pad(perCorner * 4 * (s.npt + s.nee)) : 0);
  l.total = l.friction + (s.friction ? pad(perCorner * 4 * (s.fNpt + s.fNee)) : 0);
  return l;
}

// the checks every entry has in common: each term that is present passes the checks of its own product call
inline bool system_ok(const zs_rocm_policy *pol, const zs_rocm_mesh *m, const zs_rocm_mesh_system *s) {
  if (!pol || !m || !m->stats || !s || (m->nv && !s->mass) || !(fabsf(s->scale) <= FLT_MAX)) return false;
  if (s->elastic && !elastic_args_ok(pol, m, s->mu, s->lam, s->kb)) return false;
  if (s->barrier) {
    if (!barrier_args_ok(pol, m, s->ptPairs, s->npt, s->eePairs, s->nee, s->dHat, s->kappa, s->mollify)) return false;
    if (m->nv && (!s->starts || (s->npt + s->nee && !s->entries))) return false;
  }
  if (s->friction) {
    if (!friction_args_ok(pol, m, s->u, s->fPtPairs, s->fNpt, s->fEePairs, s->fNee, s->record, s->fmu, s->epsv)) return false;
    if (m->nv && (!s->fStarts || (s->fNpt + s->fNee && !s->fEntries))) return false;
  }
  return true;
}

}  // namespace zsr
