// sf_region.hip -- regions and the groups made of them.
//   Regions             the region table of one engine, its dynamic groups, and on the device: nine program slots (eight
//                       dynamic groups and one for a static assignment or a points query) and the member counts
//   k_region_update     every dynamic group due at this step, in ONE launch: a lane loads an owned atom's position record
//                       and mask word once, walks the program of each group, and stores the word back if it changed
//                       (1024 blocks at most: beyond 262 144 atoms a lane takes several, a grid stride apart)
//   k_region_assign     group ID region RID: the atoms of the region are added to the group
//   k_region_points     sf_lammps_region_match: the match of arbitrary points
//   k_group_count       the members of any group, counted on demand
// The three match kernels call the one device function region_match (sf_region_match.h).  A program is read through a
// pointer that is the same for every lane, so the reads of its primitives and steps are uniform.
#include <algorithm>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_compute_ids.h"
#include "sf_region.h"
#include "sf_region_parse.h"

namespace sf {
namespace {

constexpr int kDynMax = 8;            // dynamic groups of one engine
constexpr int kSlotScratch = kDynMax;   // the slot of a static assignment or a points query
constexpr int kUpdateBlocks = 1024;   // the update kernel's grid is capped here: a lane takes several atoms, a block one atomic per group
constexpr int kCountStride = 1024;    // words between two member counters (4 KiB: no two of them behind one memory channel's line)
constexpr int kCounters = 2 * kDynMax + 1;   // [kDynMax] of the dynamic groups, [kDynMax] of region_cost, [1] of a count on demand

struct RegionSlot {
  int bit;         // the group's mask bit
  int parentbit;   // dynamic: only atoms of the parent can be members
  int pad[2];
  RegionProgram prog;
};

// the dynamic groups that exist, in one launch: those with update[k] are evaluated, the others only counted, so that all the
// counters can be cleared together and each is the population of its group after this launch
struct RegionDue {
  int n;
  int slot[kDynMax];
  int update[kDynMax];
};

// The member counts: a ballot's population count is the same number in every lane of the wave, so a wave keeps one running
// count per group in a register that is uniform over the wave; at the end lane 0 adds it to the block's count in LDS, and one
// thread per group adds the block's count to the group's counter -- an integer atomic per BLOCK and group, each counter in a
// 4 KiB stretch of its own.  (One atomic per wave, 15 600 of them on one address at 1 M grains, took 100 us per group: atomics
// on one line retire about 6 ns apart.  DESIGN.md section 18.)
__global__ __launch_bounds__(256) void k_region_update(const double4* __restrict__ xr, int* __restrict__ mask, int n,
                                                       const RegionSlot* __restrict__ slots, RegionDue D,
                                                       unsigned* __restrict__ count)
{
  __shared__ unsigned block_count[kDynMax];
  if (threadIdx.x < kDynMax) block_count[threadIdx.x] = 0u;
  __syncthreads();
  unsigned wave_count[kDynMax];
#pragma unroll
  for (int g = 0; g < kDynMax; g++) wave_count[g] = 0u;
  const long long stride = (long long)gridDim.x * blockDim.x;
  // (every lane of a wave makes the same number of turns -- base is the wave's first atom -- and takes part in every ballot)
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {
    const long long i = base + (threadIdx.x & 63u);
    const bool live = i < n;
    double4 x = make_double4(0.0, 0.0, 0.0, 0.0);
    int m0 = 0;
    if (live) {
      x = xr[i];
      m0 = mask[i];
    }
    int m = m0;
#pragma unroll
    for (int g = 0; g < kDynMax; g++) {
      if (g < D.n) {
        const RegionSlot& S = slots[D.slot[g]];
        bool in;
        if (D.update[g]) {
          const bool match = region_match(S.prog, x.x, x.y, x.z);
          in = live && (m0 & S.parentbit) != 0 && match;   // (a parent is never dynamic: m0 holds its bit)
          m = in ? (m | S.bit) : (m & ~S.bit);
        } else
          in = live && (m0 & S.bit) != 0;
        wave_count[g] += (unsigned)__popcll(__ballot(in));
      }
    }
    if (live && m != m0) mask[i] = m;
  }
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int g = 0; g < kDynMax; g++)
      if (g < D.n && wave_count[g]) atomicAdd(&block_count[g], wave_count[g]);
  }
  __syncthreads();
  if ((int)threadIdx.x < D.n && block_count[threadIdx.x])
    atomicAdd(&count[(size_t)kCountStride * D.slot[threadIdx.x]], block_count[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_region_assign(const double4* __restrict__ xr, int* __restrict__ mask, int n,
                                                       const RegionSlot* __restrict__ slot)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double4 x = xr[i];
  const int m = mask[i];
  if (region_match(slot->prog, x.x, x.y, x.z) && !(m & slot->bit)) mask[i] = m | slot->bit;
}

__global__ __launch_bounds__(256) void k_region_points(const double* __restrict__ xyz, int n,
                                                       const RegionSlot* __restrict__ slot, int* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* p = xyz + 3 * (size_t)i;
  out[i] = region_match(slot->prog, p[0], p[1], p[2]) ? 1 : 0;
}

// (a query, not part of a run: one atomic per wave on one address, about 100 us at 1 M atoms -- k_region_update's note)
__global__ __launch_bounds__(256) void k_group_count(const int* __restrict__ mask, int n, int bit, unsigned* __restrict__ count)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n && (mask[i] & bit) != 0;
  const unsigned long long b = __ballot(in);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned)__popcll(b));
}

struct DynGroup {
  std::string name, region;
  int bit = 0, parentbit = 0;
  long every = 1;
  int slot = 0;
  bool pending = true;   // evaluate at the beginning of the next piece of running (a new group; the setup of a `run`)
  bool counted = false;  // its device counter holds its population (a launch has evaluated or counted it since the definition)
};

struct Regions {
  RegionTable T;
  std::vector<DynGroup> dyn;
  RegionSlot h_slot[kDynMax + 1];
  RegionSlot* d_slot = nullptr;
  unsigned* d_count = nullptr;   // [kCounters] counters, kCountStride words apart
  long long launches = 0;
  // grown and kept: the points of a query and their matches, the mask copy of region_cost, the mask on its way to the host
  double* d_xyz = nullptr;
  int* d_int = nullptr;
  size_t xyz_n = 0, int_n = 0;
  ~Regions()
  {
    if (d_slot) (void)hipFree(d_slot);
    if (d_count) (void)hipFree(d_count);
    if (d_xyz) (void)hipFree(d_xyz);
    if (d_int) (void)hipFree(d_int);
  }
  DynGroup* find_dyn(const std::string& name)
  {
    for (DynGroup& g : dyn)
      if (g.name == name) return &g;
    return nullptr;
  }
};

const Regions* set_of(const SfLammps& L) { return L.regions.get<Regions>(); }
Regions& regions_of(SfLammps& L) { return L.regions.ensure<Regions>(); }

void device_ready(SfLammps& L, Regions& R)
{
  if (R.d_slot) return;
  hipStream_t st = L.eng.stream();
  SF_HIP(hipMalloc(&R.d_slot, sizeof(RegionSlot) * (kDynMax + 1)));
  SF_HIP(hipMalloc(&R.d_count, sizeof(unsigned) * kCountStride * kCounters));
  SF_HIP(hipMemsetAsync(R.d_slot, 0, sizeof(RegionSlot) * (kDynMax + 1), st));
  SF_HIP(hipMemsetAsync(R.d_count, 0, sizeof(unsigned) * kCountStride * kCounters, st));
}

// slot k of the device buffer <- the host's (at a definition, never in a run: it waits for the copy)
void slot_upload(SfLammps& L, Regions& R, int k, const RegionProgram& prog, int bit, int parentbit)
{
  device_ready(L, R);
  hipStream_t st = L.eng.stream();
  RegionSlot& S = R.h_slot[k];
  S = RegionSlot();
  S.bit = bit;
  S.parentbit = parentbit;
  S.prog = prog;
  SF_HIP(hipMemcpyAsync(R.d_slot + k, &S, sizeof(RegionSlot), hipMemcpyHostToDevice, st));
  SF_HIP(hipStreamSynchronize(st));
}

void fit_ints(SfLammps& L, Regions& R, size_t n)
{
  if (n <= R.int_n) return;
  if (R.d_int) {
    SF_HIP(hipStreamSynchronize(L.eng.stream()));
    SF_HIP(hipFree(R.d_int));
    R.d_int = nullptr;
  }
  R.int_n = n + n / 4 + 1024;
  SF_HIP(hipMalloc(&R.d_int, sizeof(int) * R.int_n));
}

// One launch for the dynamic groups chosen by `due`; the others are counted in it.  mask / count: the engine's, or the
// copies region_cost works on
void launch_update(SfLammps& L, Regions& R, const std::vector<const DynGroup*>& due, int* mask, unsigned* count)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  RegionDue D = RegionDue();
  for (const DynGroup& g : R.dyn) {
    D.slot[D.n] = g.slot;
    D.update[D.n] = std::find(due.begin(), due.end(), &g) != due.end() ? 1 : 0;
    D.n++;
  }
  SF_HIP(hipMemsetAsync(count, 0, sizeof(unsigned) * kCountStride * kDynMax, st));
  const int n = e.nlocal();
  if (!n) return;
  k_region_update<<<std::min(div_up(n, 256), kUpdateBlocks), 256, 0, st>>>(e.d_xr(), mask, n, R.d_slot, D, count);
  SF_HIP(hipGetLastError());
  R.launches++;
}

void update(SfLammps& L, Regions& R, const std::vector<const DynGroup*>& due)
{
  if (due.empty()) return;
  device_ready(L, R);
  launch_update(L, R, due, L.eng.d_mask(), R.d_count);
  for (DynGroup& g : R.dyn) g.counted = true;   // (evaluated or only counted: every group's counter is its population now)
  computes_invalidate(L);   // (membership changed at an unchanged step: the per-atom, chunk and global computes ask again)
}

const RegionDef& region_of(const Regions* R, const std::string& id, const char* missing)
{
  const RegionDef* d = R ? R->T.find(id) : nullptr;
  if (!d) fail("%s", missing);
  return *d;
}

bool engine_fix_style(const std::string& st)
{
  return st == "nve/sphere" || st == "gravity" || st == "fdrag" || st == "cohesive" || st == "freeze" || st == "wall/gran" ||
         st == "wall/granFix" || st == "rigid/nve";
}

}  // namespace

void region_command(SfLammps& L, const std::vector<std::string>& w)
{
  Regions& R = regions_of(L);
  RegionBox B;
  B.exists = L.eng.box_defined();
  if (B.exists) {
    int per[3];
    L.eng.box(B.lo, B.hi, per);
  }
  std::vector<std::string> in_use;
  for (const DynGroup& g : R.dyn) in_use.push_back(g.region);
  const std::string err = region_define(R.T, w, B, in_use);
  if (!err.empty()) fail("%s", err.c_str());
}

bool group_is_dynamic(const SfLammps& L, const std::string& name)
{
  if (const Regions* R = set_of(L))
    for (const DynGroup& g : R->dyn)
      if (g.name == name) return true;
  return false;
}

void group_region_command(SfLammps& L, const std::vector<std::string>& w)
{
  if (w.size() != 4) fail("Illegal group command");
  const RegionDef& d = region_of(set_of(L), w[3], "Group region ID does not exist");
  Regions& R = regions_of(L);
  DemEngine& e = L.eng;
  const int bit = e.group_make(w[1]);
  slot_upload(L, R, kSlotScratch, d.prog, bit, 1);
  const int n = e.nlocal();
  if (!n) return;
  k_region_assign<<<div_up(n, 256), 256, 0, e.stream()>>>(e.d_xr(), e.d_mask(), n, R.d_slot + kSlotScratch);
  SF_HIP(hipGetLastError());
  R.launches++;
}

void group_dynamic_command(SfLammps& L, const std::vector<std::string>& w)
{
  // [3P] group ID dynamic PARENT keyword value ...: region RID | var NAME | property NAME | every N
  if (w.size() < 4) fail("Illegal group command");
  const std::string& name = w[1];
  const std::string& parent = w[3];
  refuse_decomposed(L, "group dynamic");
  if (name == "all") fail("Group all cannot be made dynamic");
  if (name == parent) fail("Group dynamic cannot reference itself");
  DemEngine& e = L.eng;
  if (!e.groups().count(parent)) fail("Group dynamic parent group does not exist");
  if (group_is_dynamic(L, parent)) fail("Group dynamic parent group cannot be dynamic");
  std::string rid;
  long every = 1;
  for (size_t k = 4; k < w.size(); k += 2) {
    if (w[k] == "var" || w[k] == "property")
      fail("group dynamic: keyword %s is not supported (region and every are)", w[k].c_str());
    if (k + 1 >= w.size()) fail("Illegal group command");
    if (w[k] == "region") rid = w[k + 1];
    else if (w[k] == "every") {
      char* end = nullptr;
      every = std::strtol(w[k + 1].c_str(), &end, 10);
      if (end == w[k + 1].c_str() || *end != '\0' || every <= 0) fail("Illegal group command");
    } else
      fail("Illegal group command");
  }
  if (rid.empty()) fail("group dynamic: give region RID (var and property are not supported)");
  const RegionDef& d = region_of(set_of(L), rid, "Group region ID does not exist");
  Regions& R = regions_of(L);
  if (e.groups().count(name)) {
    const int bit = e.group_bit(name);
    if (e.fix_uses_group_bit(bit))
      fail("group %s dynamic: a fix of the sub-step kernel or the rigid integrator uses this group, and its group bit is "
           "decided once: a dynamic group is for computes, dumps and the averaging fixes", name.c_str());
    for (const DynGroup& o : R.dyn)   // ([3P] FixGroup::init refuses a dynamic parent whichever of the two came first)
      if (o.parentbit == bit)
        fail("group %s dynamic: it is the parent of the dynamic group %s, and a parent group cannot be dynamic", name.c_str(),
             o.name.c_str());
  }
  DynGroup* g = R.find_dyn(name);
  if (!g) {
    if ((int)R.dyn.size() >= kDynMax) fail("Too many dynamic groups (at most %d)", kDynMax);
    bool used[kDynMax] = {false};
    for (const DynGroup& o : R.dyn) used[o.slot] = true;
    DynGroup n;
    n.name = name;
    n.slot = (int)(std::find(used, used + kDynMax, false) - used);
    n.bit = e.group_make(name);
    R.dyn.push_back(n);
    g = &R.dyn.back();
  }
  g->region = rid;
  g->parentbit = e.group_bit(parent);
  g->every = every;
  g->pending = true;
  g->counted = false;
  slot_upload(L, R, g->slot, d.prog, g->bit, g->parentbit);
}

void group_static_command(SfLammps& L, const std::vector<std::string>& w)
{
  if (w.size() != 3) fail("Illegal group command");
  (void)L.eng.group_bit(w[1]);
  if (!L.regions) return;
  Regions& R = regions_of(L);
  for (size_t k = 0; k < R.dyn.size(); k++)
    if (R.dyn[k].name == w[1]) {
      R.dyn.erase(R.dyn.begin() + (long)k);
      return;
    }
}

void region_refuse_engine_fix(const SfLammps& L, const std::string& style, const std::string& group)
{
  if (engine_fix_style(style) && group_is_dynamic(L, group))
    fail("fix %s: %s is a dynamic group, and the group bit of this fix is decided once: give a static group (a dynamic group "
         "is for computes, dumps and the averaging fixes)", style.c_str(), group.c_str());
}

bool region_dynamic_any(const SfLammps& L)
{
  const Regions* R = set_of(L);
  return R && !R->dyn.empty();
}

long long region_next_step(const SfLammps& L, long long step)
{
  long long next = -1;
  if (const Regions* R = set_of(L))
    for (const DynGroup& g : R->dyn) {
      const long long s = (step / g.every + 1) * g.every;
      if (next < 0 || s < next) next = s;
    }
  return next;
}

void region_run_setup(SfLammps& L)
{
  if (!L.regions) return;
  for (DynGroup& g : regions_of(L).dyn) g.pending = true;
}

void region_begin_due(SfLammps& L)
{
  if (!L.regions) return;
  Regions& R = regions_of(L);
  std::vector<const DynGroup*> due;
  for (DynGroup& g : R.dyn)
    if (g.pending) {
      due.push_back(&g);
      g.pending = false;
    }
  update(L, R, due);
}

void region_step_due(SfLammps& L)
{
  if (!L.regions) return;
  Regions& R = regions_of(L);
  const long long step = L.eng.nsteps();
  std::vector<const DynGroup*> due;
  for (DynGroup& g : R.dyn)
    if (step % g.every == 0) {
      due.push_back(&g);
      g.pending = false;
    }
  update(L, R, due);
}

}  // namespace sf

using sf::handle;

extern "C" {

int sf_lammps_region_match(void* ptr, const char* id, int n, const double* xyz, int* out)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id || n < 0 || (n > 0 && (!xyz || !out))) sf::fail("sf_lammps_region_match: bad argument");
  const sf::RegionDef& d = sf::region_of(sf::set_of(L), id, "Region ID does not exist");
  if (n > 0) {
    sf::Regions& R = sf::regions_of(L);
    hipStream_t st = L.eng.stream();
    sf::slot_upload(L, R, sf::kSlotScratch, d.prog, 0, 0);
    sf::fit_ints(L, R, (size_t)n);
    if (3 * (size_t)n > R.xyz_n) {
      if (R.d_xyz) {
        SF_HIP(hipStreamSynchronize(st));
        SF_HIP(hipFree(R.d_xyz));
        R.d_xyz = nullptr;
      }
      R.xyz_n = 3 * (size_t)n + 3072;
      SF_HIP(hipMalloc(&R.d_xyz, sizeof(double) * R.xyz_n));
    }
    SF_HIP(hipMemcpyAsync(R.d_xyz, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    sf::k_region_points<<<sf::div_up(n, 256), 256, 0, st>>>(R.d_xyz, n, R.d_slot + sf::kSlotScratch, R.d_int);
    SF_HIP(hipGetLastError());
    R.launches++;
    SF_HIP(hipMemcpyAsync(out, R.d_int, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
  }
  SF_API_END(0)
}

int sf_lammps_group_mask(void* ptr, const char* name, int* out)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!name) sf::fail("sf_lammps_group_mask: null argument");
  const int bit = L.eng.group_bit(name);
  const int n = L.eng.nlocal();
  if (n > 0) {
    if (!out) sf::fail("sf_lammps_group_mask: null argument");
    hipStream_t st = L.eng.stream();
    SF_HIP(hipMemcpyAsync(out, L.eng.d_mask(), sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) out[i] = (out[i] & bit) ? 1 : 0;
  }
  SF_API_END(0)
}

long long sf_lammps_group_count(void* ptr, const char* name)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!name) sf::fail("sf_lammps_group_count: null argument");
  const int bit = L.eng.group_bit(name);
  sf::Regions& R = sf::regions_of(L);
  sf::device_ready(L, R);
  hipStream_t st = L.eng.stream();
  unsigned* c = R.d_count + (size_t)sf::kCountStride * 2 * sf::kDynMax;
  const sf::DynGroup* g = R.find_dyn(name);
  if (g && g->counted)
    c = R.d_count + (size_t)sf::kCountStride * g->slot;   // (the counter of its last evaluation)
  else {   // (any other group; a dynamic group that no launch has counted since its definition: its bits as they stand)
    SF_HIP(hipMemsetAsync(c, 0, sizeof(unsigned), st));
    const int n = L.eng.nlocal();
    if (n > 0) {
      sf::k_group_count<<<sf::div_up(n, 256), 256, 0, st>>>(L.eng.d_mask(), n, bit, c);
      SF_HIP(hipGetLastError());
    }
  }
  unsigned h = 0;
  SF_HIP(hipMemcpyAsync(&h, c, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  SF_HIP(hipStreamSynchronize(st));
  SF_API_END((long long)h)
}

int sf_lammps_region_launches(void* ptr, long long* launches)
{
  SF_API_BEGIN
  if (!launches) sf::fail("sf_lammps_region_launches: null argument");
  const sf::Regions* R = sf::set_of(*handle(ptr));
  *launches = R ? R->launches : 0;
  SF_API_END(0)
}

int sf_lammps_region_cost(void* ptr, const char* name, double* ms)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!ms) sf::fail("sf_lammps_region_cost: null argument");
  sf::Regions& R = sf::regions_of(L);
  std::vector<const sf::DynGroup*> due;
  if (name && *name) {
    const sf::DynGroup* g = R.find_dyn(name);
    if (!g) sf::fail("sf_lammps_region_cost: %s is not a dynamic group", name);
    due.push_back(g);
  } else
    for (const sf::DynGroup& g : R.dyn) due.push_back(&g);
  if (due.empty()) sf::fail("sf_lammps_region_cost: there is no dynamic group");
  // on a copy of the mask and counters of its own: the groups stay as their schedule left them
  sf::device_ready(L, R);
  const int n = L.eng.nlocal();
  hipStream_t st = L.eng.stream();
  sf::fit_ints(L, R, (size_t)std::max(n, 1));
  if (n > 0) SF_HIP(hipMemcpyAsync(R.d_int, L.eng.d_mask(), sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st));
  const long long before = R.launches;
  *ms = sf::stream_ms(st, [&] { sf::launch_update(L, R, due, R.d_int, R.d_count + (size_t)sf::kCountStride * sf::kDynMax); });
  R.launches = before;   // (a measurement, not an update)
  SF_API_END(0)
}

}  // extern "C"
