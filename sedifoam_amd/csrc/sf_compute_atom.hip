// sf_compute_atom.hip -- the per-atom computes ([3P] LAMMPS names and definitions):
//   compute ID group stress/atom [NULL] [ke] [pair] [virial] [fix] [bond] [angle] [dihedral] [improper] [kspace]
//       six columns xx yy zz xy xz yz in stress x volume units, LAMMPS' sign (nktv2p = mvv2e = 1):
//       s_ab(i) = -( [ke] m_i v_a v_b + [pair] sum_j 1/2 del_a F_b ),  del = x_i - x_j with the partner moved to the periodic
//       image the list word names, F the pair style's force on i from j (normal + tangential, the `fix freeze` meff
//       override included): the ev_tally_xyz half share under newton off, exactly the summand of k_thermo_virial
//       (sf_thermo.hip), so that the sum over all atoms is thermo's W and kinetic terms.  No keyword: ke and pair.  fix,
//       bond ... kspace add nothing: no fix here tallies a virial; walls, cohesion, drag and gravity are not in it.
//   compute ID group contact/atom          the partners j (of any group) with rsq < (radi + radj)^2
//   compute ID group ke/atom               1/2 m v^2
//   compute ID group erotate/sphere/atom   1/2 (0.4 m r^2) omega^2
//   compute ID group property/atom a1 ...  id type mass radius diameter x y z vx vy vz fx fy fz omegax omegay omegaz tqx tqy
//                                          tqz as stored; xu yu zu ix iy iz: the unwrapped coordinates and the periodic
//                                          image counts (sf_unmap.h).  One attribute a per-atom vector, several an array
//   compute ID group displace/atom         dx dy dz and their length: unmap(x) - x0, x0 the unwrapped position when the
//                                          compute was defined (of an atom created later: at its creation); DESIGN.md 17
//   compute ID group coord/atom cutoff Rc [typerange ...]   the atoms j != i (of any group) with rsq < Rc^2, per type range:
//                                          a walk of a grid of that cutoff on the positions as they stand (sf_nbr.hip;
//                                          DESIGN.md 20), not of the pair list.  One range a vector, several an array
//   compute ID group cluster/atom CUT [surface no|yes] [size no|yes]   the smallest tag of the atom's connected component,
//                                          two group atoms linked when rsq < CUT^2 ([3P] ComputeClusterAtom); [own] surface
//                                          yes: when rsq < ((ri + rj) + CUT)^2, the reach test of fix cohesive; [own] size yes:
//                                          a second column, the atoms of the component.  Union-find on the same grid
//                                          (sf_nbr.hip): several launches and one 4-byte copy per verify round
// The group selects the atoms that get a value; atoms outside it read 0.  Like compute pair/local (sf_contacts.hip) a
// value is evaluated from the state AT THE MOMENT OF THE OUTPUT -- the x v omega a dump custom frame shows, the shear
// history sf_dem_get_history returns -- with shearupdate = false, and nothing is stored back.  (LAMMPS tallies vatom inside
// the step's force evaluation, with the half-step velocities; at `run 0` the two coincide.)
//
// One launch per evaluation (coord/atom and cluster/atom: those of sf_nbr.hip), one lane per owned atom, field-major stores val[c][i]; no atomics, no LDS, no
// floating-point reduction across lanes: the same state gives the same bits.  An evaluation is kept with the step it was
// made at and shared by every dump and query of that step.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_atom_terms.h"
#include "sf_chunk.h"
#include "sf_compute_atom.h"
#include "sf_compute_ids.h"
#include "sf_compute_parse.h"
#include "sf_dem_dispatch.h"
#include "sf_displace.h"
#include "sf_displace_parse.h"
#include "sf_global_parse.h"
#include "sf_handles.h"
#include "sf_nbr.h"

namespace sf {
namespace {

__device__ __forceinline__ Vec3 av3(const double4& a) { return {a.x, a.y, a.z}; }

// The neighbour loop of k_thermo_virial (sf_thermo.hip) with shearupdate = false, keeping the atom's own six sums: the
// same list words (root + image code, or plain index with ghost atoms), the pair's history from this side's slot where
// the word carries kOwnBit, from the owner's slot negated where it does not, zero without the touch bit.
template <int STYLE>
__global__ __launch_bounds__(256) void k_atom_virial(DemPtrs P, StepParams S, const int* mask, int groupbit, int ke, int pair,
                                                     double* val)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.nlocal) return;
  const size_t n = (size_t)S.nlocal, cap = (size_t)S.cap;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (mask[i] & groupbit) {
    const double4 xi4 = P.xr_in[i], vi4 = P.vm_in[i], wi4 = P.om_in[i];
    const Vec3 xi = av3(xi4), vi = av3(vi4), wi = av3(wi4);
    const double radi = xi4.w, mi = vi4.w;
    const int nn = pair ? P.numneigh[i] : 0;
    for (int s = 0; s < nn; s++) {
      const int jraw = P.neigh[(size_t)s * cap + i];
      const int j = neigh_index(jraw, S.roots);
      const bool own = (jraw & kOwnBit) != 0;
      double4 xj4 = P.xr_in[j];
      if (S.roots && own) shift_to_image(xj4, jraw, S.prd);
      const Vec3 del = xi - av3(xj4);
      const double rsq = dot(del, del);
      const double radj = xj4.w;
      const double radsum = radi + radj;
      if (!(rsq < radsum * radsum)) continue;
      const double4 vj4 = P.vm_in[j], wj4 = P.om_in[j];
      Vec3 sh = {0.0, 0.0, 0.0};
      if (jraw & kTouchBit) {
        if (own) {
          const double* hin = P.shear_in + (size_t)(3 * s) * cap;
          sh = {hin[i], hin[cap + i], hin[2 * cap + i]};
        } else {   // the owner's value, seen from this side
          const double* src = P.shear_in + (size_t)(3 * ((jraw >> kIdxBits) & 31)) * cap + (size_t)(jraw & kIdxMask);
          sh = {-src[0], -src[cap], -src[2 * cap]};
        }
      }
      ContactIn c;
      c.del = del;
      c.rsq = rsq;
      sf_sqrt_rsqrt(rsq, c.r, c.rinv);
      c.vr = vi - av3(vj4);
      c.wsum = {radi * wi.x + radj * wj4.x, radi * wi.y + radj * wj4.y, radi * wi.z + radj * wj4.z};
      const double mj = vj4.w;
      const PairScales m = pair_scales(mi, mj, radi, radj, c.r);
      c.overlap = m.overlap;
      c.meff = m.meff;
      c.reff = m.reff;
      if (S.freeze_bit) {   // pair_gran_hertzFix_history.cpp:188-189
        if (wi4.w != 0.0) c.meff = mj;
        if (wj4.w != 0.0) c.meff = mi;
      }
      ContactOut o;
      gran_history_law<STYLE>(S.gran, S.dt, false, c, sh, o);
      v[0] += 0.5 * del.x * o.F.x;
      v[1] += 0.5 * del.y * o.F.y;
      v[2] += 0.5 * del.z * o.F.z;
      v[3] += 0.5 * del.x * o.F.y;
      v[4] += 0.5 * del.x * o.F.z;
      v[5] += 0.5 * del.y * o.F.z;
    }
    if (ke) {
      v[0] += mi * vi.x * vi.x;
      v[1] += mi * vi.y * vi.y;
      v[2] += mi * vi.z * vi.z;
      v[3] += mi * vi.x * vi.y;
      v[4] += mi * vi.x * vi.z;
      v[5] += mi * vi.y * vi.z;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) v[c] = -v[c];
  }
#pragma unroll
  for (int c = 0; c < 6; c++) val[(size_t)c * n + i] = v[c];
}

// the same walk, gathering only what the touch test needs: the partner's record
__global__ __launch_bounds__(256) void k_atom_contacts(DemPtrs P, StepParams S, const int* mask, int groupbit, double* val)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.nlocal) return;
  int count = 0;
  if (mask[i] & groupbit) {
    const size_t cap = (size_t)S.cap;
    const double4 xi4 = P.xr_in[i];
    const Vec3 xi = av3(xi4);
    const int nn = P.numneigh[i];
    for (int s = 0; s < nn; s++) {
      const int jraw = P.neigh[(size_t)s * cap + i];
      double4 xj4 = P.xr_in[neigh_index(jraw, S.roots)];
      if (S.roots && (jraw & kOwnBit)) shift_to_image(xj4, jraw, S.prd);
      const Vec3 del = xi - av3(xj4);
      const double radsum = xi4.w + xj4.w;
      count += dot(del, del) < radsum * radsum ? 1 : 0;
    }
  }
  val[i] = (double)count;
}

// rot = 0: 1/2 m v^2;  rot = 1: 1/2 (0.4 m r^2) omega^2  ([3P] ComputeERotateSphereAtom, INERTIA = 0.4)
__global__ __launch_bounds__(256) void k_atom_kinetic(const double4* xr, const double4* vm, const double4* om, const int* mask,
                                                      int groupbit, int rot, int n, double* val)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double e = 0.0;
  if (mask[i] & groupbit) {
    const double4 v = vm[i];
    if (rot) {
      const double4 w = om[i];
      const double r = xr[i].w;
      e = atom_erotate_term(v, w, r);
    } else
      e = atom_ke_term(v);
  }
  val[i] = e;
}

// the attributes of compute property/atom, as the state records hold them
struct PropCols {
  int n;
  int a[kPropMaxAttrs];
};
__global__ __launch_bounds__(256) void k_atom_property(const double4* xr, const double4* vm, const double4* om,
                                                       const double4* force, const double4* torque, const int* tag,
                                                       const int* type, const int* mask, int groupbit, PropCols C, int n,
                                                       ImageView V, double* val)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool in = (mask[i] & groupbit) != 0;
  int im[3] = {0, 0, 0};
  double xu[3] = {0.0, 0.0, 0.0};
  if (V.image && in) {   // (null: no attribute of this compute needs it)
    image_of(V, tag[i], im);
    unmap(xr[i], im, V, xu);
  }
  const double4 zero = make_double4(0.0, 0.0, 0.0, 0.0);
  const double4 x = in ? xr[i] : zero, v = in ? vm[i] : zero, w = in ? om[i] : zero, f = in ? force[i] : zero,
                t = in ? torque[i] : zero;
  const double id = in ? (double)tag[i] : 0.0, ty = in ? (double)type[i] : 0.0;
#pragma unroll
  for (int k = 0; k < kPropMaxAttrs; k++) {
    if (k < C.n) {
      double o = 0.0;
      switch (C.a[k]) {
        case PA_ID: o = id; break;
        case PA_TYPE: o = ty; break;
        case PA_MASS: o = v.w; break;
        case PA_RADIUS: o = x.w; break;
        case PA_DIAMETER: o = 2.0 * x.w; break;
        case PA_X: o = x.x; break;
        case PA_Y: o = x.y; break;
        case PA_Z: o = x.z; break;
        case PA_VX: o = v.x; break;
        case PA_VY: o = v.y; break;
        case PA_VZ: o = v.z; break;
        case PA_FX: o = f.x; break;
        case PA_FY: o = f.y; break;
        case PA_FZ: o = f.z; break;
        case PA_OMEGAX: o = w.x; break;
        case PA_OMEGAY: o = w.y; break;
        case PA_OMEGAZ: o = w.z; break;
        case PA_TQX: o = t.x; break;
        case PA_TQY: o = t.y; break;
        case PA_TQZ: o = t.z; break;
        case PA_XU: o = xu[0]; break;
        case PA_YU: o = xu[1]; break;
        case PA_ZU: o = xu[2]; break;
        case PA_IX: o = (double)im[0]; break;
        case PA_IY: o = (double)im[1]; break;
        default: o = (double)im[2]; break;
      }
      val[(size_t)k * (size_t)n + i] = o;
    }
  }
}

// dx dy dz |d| of compute displace/atom: d = unmap(x) - x0[tag], each component one rounded difference
__global__ __launch_bounds__(256) void k_atom_displace(const double4* xr, const int* tag, const int* mask, int groupbit, int n,
                                                       ImageView V, const double* x0, int rows, double* val)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double d[3] = {0.0, 0.0, 0.0};
  const int t = tag[i];
  if ((mask[i] & groupbit) && t >= 0 && t < rows) {
    int im[3];
    double xu[3];
    image_of(V, t, im);
    unmap(xr[i], im, V, xu);
    const double* r = x0 + 3 * (size_t)t;
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = sub_rn(xu[k], r[k]);
  }
  const size_t N = (size_t)n;
  val[i] = d[0];
  val[N + i] = d[1];
  val[2 * N + i] = d[2];
  val[3 * N + i] = length_rn(d[0], d[1], d[2]);
}

// ---- host side ----

enum Kind { K_STRESS, K_CONTACT, K_KE, K_EROTATE, K_PROPERTY, K_DISPLACE, K_COORD, K_CLUSTER };
constexpr int kNumKinds = 8;
const char* const kStyleName[kNumKinds] = {"stress/atom", "contact/atom", "ke/atom", "erotate/sphere/atom", "property/atom",
                                           "displace/atom", "coord/atom", "cluster/atom"};

struct AtomCompute {
  std::string id;
  Kind kind = K_KE;
  int groupbit = 1;
  bool ke = true, pair = true;
  std::vector<int> attrs;   // K_PROPERTY
  RefTable ref;             // K_DISPLACE: the reference positions, by tag
  CoordSpec coord;          // K_COORD: the cutoff and the type ranges
  ClusterSpec cluster;      // K_CLUSTER: the cutoff, the link rule and whether the size column exists
  ClusterWork cluster_work; // K_CLUSTER: the union-find scratch, kept like val, and the verify rounds of the last evaluation
  DeviceScratch val;
  StateStamp made;   // what the buffer was made at
  int ncols() const
  {
    if (kind == K_COORD) return (int)coord.ranges.size();
    if (kind == K_CLUSTER) return cluster.size ? 2 : 1;
    return kind == K_STRESS ? 6 : (kind == K_PROPERTY ? (int)attrs.size() : (kind == K_DISPLACE ? 4 : 1));
  }
  bool needs_image() const
  {
    if (kind == K_DISPLACE) return true;
    for (int a : attrs)
      if (kind == K_PROPERTY && prop_attr_needs_image(a)) return true;
    return false;
  }
  std::string who() const;
};

struct AtomSet {
  std::vector<std::unique_ptr<AtomCompute>> computes;
  long long launches = 0;
  AtomCompute* find(const std::string& id)
  {
    for (auto& c : computes)
      if (c->id == id) return c.get();
    return nullptr;
  }
};

std::string AtomCompute::who() const { return std::string("compute ") + kStyleName[kind]; }

AtomSet* set_of(const SfLammps& L) { return L.atom_computes.get<AtomSet>(); }
AtomSet& ensure_set(SfLammps& L) { return L.atom_computes.ensure<AtomSet>(); }

// what an evaluation needs of the engine as it is now (checked at the compute line and at every evaluation: the pair
// style and the fixes may have changed since)
void refuse_unsupported(const SfLammps& L, Kind kind)
{
  const DemEngine& e = L.eng;
  refuse_decomposed(L, (std::string("compute ") + kStyleName[kind]).c_str());
  if (kind == K_STRESS) {
    if (e.pair_lubricate_on())
      fail("compute stress/atom: not with lubricate/poly in the pair style (its pair terms are not in the per-atom stress)");
    if (e.pair_gran_style() == 0)
      fail("compute stress/atom: no granular pair style is defined (the per-atom virial is that of the contact law)");
    if (e.rigid_on())
      fail("compute stress/atom: not while fix rigid/nve exists (the pair law then takes the masses of the bodies)");
  } else if (kind == K_CONTACT) {
    if (e.pair_gran_style() == 0 && !e.pair_lubricate_on())
      fail("compute contact/atom: no pair style is defined (a pair style builds the neighbour list it counts in)");
  }
}

void evaluate(SfLammps& L, AtomSet& T, AtomCompute& c)
{
  refuse_unsupported(L, c.kind);
  DemEngine& e = L.eng;
  const int n = e.nlocal();
  hipStream_t st = e.stream();
  double* val = static_cast<double*>(c.val.get(sizeof(double) * (size_t)c.ncols() * (size_t)std::max(n, 1), st));
  if (c.kind == K_COORD) {   // (the grid and the walk are launches of sf_nbr.hip, counted there)
    nbr_coord_atom(L, "compute coord/atom", c.groupbit, c.coord.rc, c.coord.ranges, val);
  } else if (c.kind == K_CLUSTER) {
    nbr_cluster_atom(L, "compute cluster/atom", c.groupbit, c.cluster, c.cluster_work, val);
  } else if (n > 0) {
    const unsigned nb = (unsigned)div_up(n, 256);
    if (c.kind == K_KE || c.kind == K_EROTATE) {
      k_atom_kinetic<<<nb, 256, 0, st>>>(e.d_xr(), e.d_vm(), e.d_om(), e.d_mask(), c.groupbit, c.kind == K_EROTATE ? 1 : 0, n,
                                         val);
    } else if (c.kind == K_PROPERTY) {
      PropCols C{};
      C.n = (int)c.attrs.size();
      for (int k = 0; k < C.n; k++) C.a[k] = c.attrs[k];
      ImageView V{};   // (image = nullptr: not needed)
      if (c.needs_image()) V = image_view(L, c.who().c_str());
      k_atom_property<<<nb, 256, 0, st>>>(e.d_xr(), e.d_vm(), e.d_om(), e.d_force(), e.d_torque(), e.d_tag(), e.d_type(),
                                          e.d_mask(), c.groupbit, C, n, V, val);
    } else if (c.kind == K_DISPLACE) {
      const ImageView V = image_view(L, c.who().c_str());
      c.ref.fit(e);
      k_atom_displace<<<nb, 256, 0, st>>>(e.d_xr(), e.d_tag(), e.d_mask(), c.groupbit, n, V, c.ref.x0, (int)c.ref.rows, val);
    } else {
      DemPtrs P;
      StepParams S;
      if (!e.contact_view(&P, &S))
        fail("compute %s: no neighbour list yet (the contacts are those of the last force evaluation: run 0 first)",
             kStyleName[c.kind]);
      if (S.nlocal != n) fail("compute %s: the list does not describe the owned atoms", kStyleName[c.kind]);
      if (c.kind == K_CONTACT) k_atom_contacts<<<nb, 256, 0, st>>>(P, S, e.d_mask(), c.groupbit, val);
      else {
        const int ke = c.ke ? 1 : 0, pair = c.pair ? 1 : 0;
        const int groupbit = c.groupbit;
        const int* mask = e.d_mask();
        // (plain gran/hooke, GranParams::style 3, runs the Hookean instantiation: the law branches on the style itself)
        style_dispatch(S.gran.style, [&](auto style) {
          constexpr int ST = decltype(style)::value == 2 ? 2 : 1;
          k_atom_virial<ST><<<nb, 256, 0, st>>>(P, S, mask, groupbit, ke, pair, val);
        });
      }
    }
    SF_HIP(hipGetLastError());
    T.launches++;
  }
  c.made.set(e);
}

// ---- the kind (sf_compute_ids.h) ----

bool is_style(const std::string& style)
{
  if (style == "chunk/atom") return true;   // (the fifth per-atom style: sf_chunk.hip holds it, the functions below forward)
  if (!cluster_unsupported_style(style).empty()) return true;   // (refused by name in define)
  for (const char* s : kStyleName)
    if (style == s) return true;
  return false;
}

void define(SfLammps& L, const std::vector<std::string>& w)
{
  if (w[3] == "chunk/atom") {
    chunk_compute_define(L, w);
    return;
  }
  fail_if(cluster_unsupported_style(w[3]));
  auto c = std::make_unique<AtomCompute>();
  c->id = w[1];
  c->groupbit = L.eng.group_bit(w[2]);
  for (int k = 0; k < kNumKinds; k++)
    if (w[3] == kStyleName[k]) c->kind = (Kind)k;
  if (c->kind == K_STRESS) {
    const std::string err = parse_stress_keywords(w, 4, &c->ke, &c->pair);
    if (!err.empty()) fail("%s", err.c_str());
  } else if (c->kind == K_PROPERTY) {
    const std::string err = parse_property_atom(w, &c->attrs);
    if (!err.empty()) fail("%s", err.c_str());
  } else if (c->kind == K_DISPLACE) {
    const std::string err = parse_displace_atom(w);
    if (!err.empty()) fail("%s", err.c_str());
  } else if (c->kind == K_COORD) {
    const std::string err = parse_coord_atom(w, &c->coord);
    if (!err.empty()) fail("%s", err.c_str());
  } else if (c->kind == K_CLUSTER) {
    fail_if(parse_cluster_atom(w, &c->cluster));
  } else if (w.size() != 4)
    fail("Illegal compute %s command", w[3].c_str());
  refuse_unsupported(L, c->kind);
  if (c->needs_image()) {
    const ImageView V = image_view(L, c->who().c_str());   // (refused where image counts cannot be kept; makes the table)
    if (c->kind == K_DISPLACE) ref_set_all(L, c->ref, V);
  }
  ensure_set(L).computes.push_back(std::move(c));
}

bool shape(const SfLammps& L, const std::string& id, ComputeShape* s)
{
  AtomSet* T = set_of(L);
  const AtomCompute* c = T ? T->find(id) : nullptr;
  if (!c) return chunk_compute_shape(L, id, s);
  *s = ComputeShape();
  s->kind = CK_PERATOM;
  s->n = c->ncols();
  return true;
}

void remove(SfLammps& L, const std::string& id)
{
  chunk_compute_remove(L, id);
  if (AtomSet* T = set_of(L)) compute_take(L, T->computes, id);   // (a frame queued on the stream may still read its buffer)
}

void invalidate(SfLammps& L)
{
  if (AtomSet* T = set_of(L))
    for (auto& c : T->computes) c->made.clear();
}

}  // namespace

const ComputeKindOps& atom_compute_kind()
{
  static const ComputeKindOps kind = {is_style, define, remove, shape, invalidate};
  return kind;
}

const double* atom_compute_values(SfLammps& L, const std::string& id, int* ncols)
{
  AtomSet* T = set_of(L);
  AtomCompute* c = T ? T->find(id) : nullptr;
  if (!c) {
    fail_if(check_get_atom(compute_shape(L, id), id));
    if (ncols) *ncols = 1;   // (a per-atom compute that is not held here: chunk/atom)
    return chunk_compute_values(L, id);
  }
  if (!c->made.is_now(L.eng)) evaluate(L, *T, *c);
  else refuse_unsupported(L, c->kind);
  if (ncols) *ncols = c->ncols();
  return static_cast<const double*>(c->val.p);
}

bool atom_compute_coord_spec(const SfLammps& L, const std::string& id, int* groupbit, double* rc, std::vector<TypeRange>* ranges)
{
  AtomSet* T = set_of(L);
  const AtomCompute* c = T ? T->find(id) : nullptr;
  if (!c || c->kind != K_COORD) return false;
  *groupbit = c->groupbit;
  *rc = c->coord.rc;
  *ranges = c->coord.ranges;
  return true;
}

ClusterWork* atom_compute_cluster_spec(const SfLammps& L, const std::string& id, int* groupbit, ClusterSpec* spec)
{
  AtomSet* T = set_of(L);
  AtomCompute* c = T ? T->find(id) : nullptr;
  if (!c || c->kind != K_CLUSTER) return nullptr;
  if (groupbit) *groupbit = c->groupbit;
  if (spec) *spec = c->cluster;
  return &c->cluster_work;
}

bool atom_compute_tracks_created(const SfLammps& L)
{
  if (const AtomSet* T = set_of(L))
    for (const auto& c : T->computes)
      if (c->kind == K_DISPLACE) return true;
  return false;
}

void atom_compute_created(SfLammps& L, const int* d_tags, int np)
{
  AtomSet* T = set_of(L);
  if (!T) return;
  for (auto& c : T->computes)
    if (c->kind == K_DISPLACE) ref_set_tags(L, c->ref, image_view(L, c->who().c_str()), d_tags, np);
}

long long atom_compute_launches(const SfLammps& L)
{
  const AtomSet* T = set_of(L);
  return T ? T->launches : 0;
}

double atom_compute_cost(SfLammps& L, const std::string& id)
{
  fail_if(check_atom_cost(compute_shape(L, id), id));
  AtomSet* T = set_of(L);
  AtomCompute* c = T->find(id);
  hipStream_t st = L.eng.stream();
  c->val.get(sizeof(double) * (size_t)c->ncols() * (size_t)std::max(L.eng.nlocal(), 1), st);   // (not in the time)
  return stream_ms(st, [&] { evaluate(L, *T, *c); });
}

}  // namespace sf

using sf::handle;

extern "C" {

long long sf_lammps_compute_atom(void* ptr, const char* id, long long max, int* tag, double* values, int* ncols)
{
  long long n = 0;
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id) sf::fail("sf_lammps_compute_atom: null argument");
  int nc = 0;
  const double* d_val = sf::atom_compute_values(L, id, &nc);
  if (ncols) *ncols = nc;
  n = L.eng.nlocal();
  if (n > 0 && n <= max) {
    if (!tag || !values) sf::fail("sf_lammps_compute_atom: null argument");
    hipStream_t st = L.eng.stream();
    std::vector<double> cols((size_t)nc * (size_t)n);
    SF_HIP(hipMemcpyAsync(tag, L.eng.d_tag(), sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(cols.data(), d_val, sizeof(double) * cols.size(), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    for (long long r = 0; r < n; r++)   // field-major on the device, row-major for the caller
      for (int c = 0; c < nc; c++) values[(size_t)nc * (size_t)r + c] = cols[(size_t)c * (size_t)n + (size_t)r];
  }
  SF_API_END(n)
}

int sf_lammps_compute_atom_launches(void* ptr, long long* launches)
{
  SF_API_BEGIN
  if (!launches) sf::fail("sf_lammps_compute_atom_launches: null argument");
  *launches = sf::atom_compute_launches(*handle(ptr));
  SF_API_END(0)
}

int sf_lammps_compute_atom_cost(void* ptr, const char* id, double* ms)
{
  SF_API_BEGIN
  if (!id || !ms) sf::fail("sf_lammps_compute_atom_cost: null argument");
  *ms = sf::atom_compute_cost(*handle(ptr), id);
  SF_API_END(0)
}

}  // extern "C"
