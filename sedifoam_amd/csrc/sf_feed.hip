// sf_feed.hip -- the device side of the cloud's particle add / delete schedules (enhancedCloud.C:694-711, 1015-1294;
// softParticleCloud.C:1099-1268), see DESIGN.md section 19:
//   k_feed_mark     one lane per owned atom: type-1 grains inside clearInitialBox / deleteParticleBox -> the engine's leave_
//                   words, both counts and the largest surviving tag; integers only, one atomic per block and counter
//   k_feed_create   one lane per new grain: every row a created atom has, written at offset nlocal_
// The host keeps the sequence of lammps_delete_particle / lammps_create_particle around them (DemEngine::compact_marked,
// create_rows_begin / create_rows_end), so a fed run is the run a host that made the same calls would see, bit for bit.
#include "sf_feed.h"

#include <climits>

#include "sf_dem.h"
#include "sf_physics.h"
#include "sf_rigid.h"

namespace sf {

__global__ __launch_bounds__(256) void k_feed_mark(int n, const double4* __restrict__ xr, const int* __restrict__ type,
                                                   const int* __restrict__ tag, FeedMark m, int* __restrict__ leave,
                                                   int* __restrict__ counters)
{
  __shared__ int ws[4][3];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool cleared = false, deleted = false;
  int keep_tag = 0;
  if (i < n) {
    const int t = tag[i];
    if (t <= m.tag_limit) {
      const double4 x = xr[i];
      if (type[i] == 1) {   // enhancedCloud.C:1105, :1210: p.ptype() == 1
        cleared = m.clear && point_in_region(m.option, m.clearBox, m.ecc, x.x, x.y, x.z);
        deleted = !cleared && m.del && point_in_region(m.option, m.deleteBox, m.ecc, x.x, x.y, x.z);
      }
      if (!cleared) keep_tag = t;   // addParticleOpenFOAM's maxTag_ (:1017-1028) runs over what the clearing left
    }
    leave[i] = (m.flag_cleared ? cleared : deleted) ? 1 : 0;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nc = __popcll(__ballot(cleared)), nd = __popcll(__ballot(deleted));
  int mt = keep_tag;
  for (int off = 32; off > 0; off >>= 1) mt = max(mt, __shfl_down(mt, off, 64));
  if (lane == 0) {
    ws[w][0] = nc;
    ws[w][1] = nd;
    ws[w][2] = mt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = ws[0][0] + ws[1][0] + ws[2][0] + ws[3][0], d = ws[0][1] + ws[1][1] + ws[2][1] + ws[3][1];
    const int t = max(max(ws[0][2], ws[1][2]), max(ws[2][2], ws[3][2]));
    if (c) atomicAdd(&counters[0], c);
    if (d) atomicAdd(&counters[1], d);
    if (t) atomicMax(&counters[2], t);
  }
}

FeedCounts DemEngine::feed_mark(const FeedMark& m)
{
  static_assert(F_FEED_DELETED == F_FEED_CLEARED + 1 && F_FEED_MAXTAG == F_FEED_CLEARED + 2 && F_FEED_MAXTAG < F_ARRIVAL,
                "the feed's three flag words are adjacent and in front of the arrival word");
  FeedCounts out{0, 0, 0};
  if (have_subdomain_) fail("the cloud's add / delete schedules: one rank only (no decomposed domain)");
  if (!nlocal_) return out;
  reset_flags(F_FEED_CLEARED, 3, 0);
  k_feed_mark<<<div_up(nlocal_, 256), 256, 0, stream_>>>(nlocal_, xr_[cur_].as<double4>(), type_.as<int>(), tag_.as<int>(), m,
                                                        leave_.as<int>(), d_flags_ + F_FEED_CLEARED);
  SF_HIP(hipGetLastError());
  read_flags();
  out.cleared = h_flags_[F_FEED_CLEARED];
  out.deleted = h_flags_[F_FEED_DELETED];
  out.maxtag = h_flags_[F_FEED_MAXTAG];
  return out;
}

struct FeedRows {   // where a created atom's rows start (offset nlocal_ applied), [rows][cap] arrays with their stride
  double4 *xr, *vm, *om, *force, *torque;
  int *tag, *type, *mask, *foamCpuId, *numneigh;
  double *fdrag, *DuDt, *vOld, *rigid, *extra;
  unsigned char* wtouch;
  size_t cap;
  int nrigid, nextra;
  double extra_init[DemEngine::kMaxExtra];
};

// position = centre + randomPerturb * (0.5 - u), u = draw 3 i + c of drand48 after srand48(seed): rounded operation by
// operation, whatever the file is compiled with
__device__ __forceinline__ double feed_coordinate(double centre, double perturb, double u)
{
#pragma clang fp contract(off)
  const double h = 0.5 - u;
  const double p = perturb * h;
  return centre + p;
}

__global__ __launch_bounds__(256) void k_feed_create(FeedCreate c, FeedRows R)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.np) return;
  Lcg48 g(c.seed);
  g.skip(3ull * (uint64_t)i);
  double p[3];
  for (int k = 0; k < 3; k++) p[k] = feed_coordinate(c.centres[3 * i + k], c.perturb, g.next());
  const double4 zero = {0.0, 0.0, 0.0, 0.0};
  R.xr[i] = {p[0], p[1], p[2], c.radius};
  R.vm[i] = {c.vel[0], c.vel[1], c.vel[2], c.mass};
  R.om[i] = zero;
  R.force[i] = zero;
  R.torque[i] = zero;
  R.tag[i] = c.first_tag + i;
  R.type[i] = c.type;
  R.mask[i] = c.mask;
  R.foamCpuId[i] = 0;
  R.numneigh[i] = 0;
  for (int k = 0; k < 3; k++) {
    R.fdrag[(size_t)k * R.cap + i] = 0.0;
    R.DuDt[(size_t)k * R.cap + i] = 0.0;
    R.vOld[(size_t)k * R.cap + i] = 0.0;
  }
  for (int r = 0; r < R.nrigid; r++) R.rigid[(size_t)r * R.cap + i] = 0.0;
  R.wtouch[i] = 0;
  for (int r = 0; r < R.nextra; r++) R.extra[(size_t)r * R.cap + i] = R.extra_init[r];
}

void DemEngine::feed_create(const FeedCreate& c)
{
  if (c.np <= 0) return;
  if (have_subdomain_) fail("the cloud's add / delete schedules: one rank only (no decomposed domain)");
  const bool stage_first = create_rows_begin(c.np, c.radius);   // (capacity for nlocal_ + np rows and more: the launch below
                                                                // writes rows nlocal_ .. nlocal_ + np - 1 of every array)
  if ((size_t)nlocal_ + (size_t)c.np > cap_) fail("feed_create: %d + %d atoms, capacity %zu", nlocal_, c.np, cap_);
  max_tag_ = std::max(max_tag_, c.first_tag + c.np - 1);
  FeedRows R;
  const size_t o = (size_t)nlocal_;
  R.xr = xr_[cur_].as<double4>() + o;
  R.vm = vm_[cur_].as<double4>() + o;
  R.om = om_[cur_].as<double4>() + o;
  R.force = force_.as<double4>() + o;
  R.torque = torque_.as<double4>() + o;
  R.tag = tag_.as<int>() + o;
  R.type = type_.as<int>() + o;
  R.mask = mask_.as<int>() + o;
  R.foamCpuId = foamCpuId_.as<int>() + o;
  R.numneigh = numneigh_.as<int>() + o;
  R.fdrag = fdrag_.as<double>() + o;
  R.DuDt = DuDt_.as<double>() + o;
  R.vOld = vOld_.as<double>() + o;
  // (fix property/atom mol without a rigid fix: the new atoms are in no molecule; with the fix the caller refuses)
  R.nrigid = rigid_rows_.ptr ? kRigidRows : 0;
  R.rigid = R.nrigid ? rigid_rows_.as<double>() + o : nullptr;
  R.wtouch = wtouch_.as<unsigned char>() + o;
  R.nextra = nextra_;   // client rows: the value registered for atoms that did not exist before
  R.extra = extra_.as<double>() + o;
  for (int r = 0; r < kMaxExtra; r++) R.extra_init[r] = extra_init_[r];
  R.cap = cap_;
  k_feed_create<<<div_up(c.np, 256), 256, 0, stream_>>>(c, R);
  SF_HIP(hipGetLastError());
  create_rows_end(c.np, stage_first);
}

}  // namespace sf
