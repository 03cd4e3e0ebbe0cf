// sf_thermo.hip -- thermo output: `thermo N`, `thermo_style one | custom kw...`, `thermo_modify norm | flush | lost error`,
// `units`, `log FILE [append] | none`, `echo`, and -screen / -log of sf_lammps_open.
//
// What a line holds ([3P] LAMMPS Thermo, ComputeTemp, ComputePressure):
//   temp  = sum m v^2 mvv2e / (dof boltz), dof = 3 natoms - 3      ke = 1/2 sum m v^2 (/ natoms under norm yes)
//   press = (sum m v^2 + W_xx + W_yy + W_zz) / (3 V)               p_ab = (sum m v_a v_b + W_ab) / V
//   W_ab  = sum over owned i and listed j of 1/2 del_ij,a F_i<-j,b (ev_tally_xyz, newton off): the pair styles' forces
//           only (granular normal + tangential, the lubricate/poly pair terms), never the fixes
//   pe = epair = evdwl = ecoul = emol = 0: none of the pair styles or fixes here tallies an energy
//           (pair_gran_hertzFix_history.cpp:282, pair_lubricate_poly.cpp:403), so etotal = ke
//   fmax = max |f component|, fnorm = sqrt(sum f.f) over the total force array.
// Schedule ([3P] Output::setup / Output::write): a header and a line at the setup of every run, a line at every multiple
// of N inside it and at its last step, never two at one step of a run; `Loop time of ...` after it.
//
// GPU side: k_thermo_virial runs in front of the sub-step launch that evaluates a thermo step's forces and tallies the
// pair virial of exactly that evaluation (same inputs, same contact laws of sf_physics.h, nothing written but per-block
// partials); k_thermo_reduce sums the kinetic tensor and the force norms per block, and one block folds every partial row
// in a fixed order -- no floating-point atomics, so a line is the same bits from run to run.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sedifoam_amd.h"
#include "sf_block_reduce.h"
#include "sf_compute_ids.h"
#include "sf_dem_dispatch.h"
#include "sf_env.h"
#include "sf_global.h"
#include "sf_global_parse.h"
#include "sf_handles.h"
#include "sf_thermo.h"

namespace sf {

namespace {

constexpr int kThermoBlock = 256;
constexpr int kVirialMaxBlocks = 2048;
constexpr int kReduceMaxBlocks = 1024;
constexpr int kKinRow = 8;    // partial row of k_thermo_reduce: m vx vx, m vy vy, m vz vz, m vx vy, m vx vz, m vy vz, f.f, max |f|
constexpr int kResult = 14;   // the final pass: kinetic tensor (6), f.f, virial (6), max |f|

__device__ __forceinline__ Vec3 tv3(const double4& a) { return {a.x, a.y, a.z}; }

// NV values per thread -> one row per block at out (sf_block_reduce.h): the first NV - NMAX components are sums, the last
// NMAX maxima.  Fixed order throughout.
template <int NV, int NMAX>
__device__ __forceinline__ void block_reduce_store(double (&v)[NV], double* out)
{
  sf::block_reduce_store<kThermoBlock, NV>(v, out, NV, [](int c, double a, double b) { return c < NV - NMAX ? a + b : fmax(a, b); });
}

// The pair virial of one force evaluation: the neighbour loop of substep_particle (sf_dem_kernels.h) without its
// stores -- same list words (root + image code, or plain index with ghost atoms), same history as that launch reads it,
// same contact laws with the same shearupdate -- keeping 1/2 del (x) F of every pair force instead of the force.
template <int STYLE, bool LUB>
__global__ __launch_bounds__(kThermoBlock) void k_thermo_virial(DemPtrs P, StepParams S, double* out)
{
  const size_t cap = (size_t)S.cap;
  const bool shearupdate = (S.mode != 2);
  const double lub_cutsq = S.lub.cut_global * S.lub.cut_global;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < S.nlocal; i += gridDim.x * blockDim.x) {
    const double4 xi4 = P.xr_in[i], vi4 = P.vm_in[i], wi4 = P.om_in[i];
    const Vec3 xi = tv3(xi4), vi = tv3(vi4), wi = tv3(wi4);
    const double radi = xi4.w, mi = vi4.w;
    const int nn = P.numneigh[i];
    for (int s = 0; s < nn; s++) {
      const int jraw = P.neigh[(size_t)s * cap + i];
      const int j = neigh_index(jraw, S.roots);
      const bool own = (jraw & kOwnBit) != 0;
      double4 xj4 = P.xr_in[j];
      if (S.roots && own) shift_to_image(xj4, jraw, S.prd);
      const Vec3 del = xi - tv3(xj4);
      const double rsq = dot(del, del);
      const double radj = xj4.w;
      const double radsum = radi + radj;
      const bool contact = STYLE != 0 && rsq < radsum * radsum;
      const bool lub = LUB && S.lub.flagHI && rsq < lub_cutsq;
      if (!contact && !lub) continue;
      const double4 vj4 = P.vm_in[j], wj4 = P.om_in[j];
      double r_pair, rinv_pair;
      sf_sqrt_rsqrt(rsq, r_pair, rinv_pair);
      Vec3 Fp = {0.0, 0.0, 0.0};
      if (contact) {
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
        c.r = r_pair;
        c.rinv = rinv_pair;
        c.vr = vi - tv3(vj4);
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
        gran_history_law<STYLE == 0 ? 1 : STYLE>(S.gran, S.dt, shearupdate, c, sh, o);
        Fp = o.F;
      }
      if (lub) {
        Vec3 T = {0.0, 0.0, 0.0};
        lubricate_poly_pair(S.lub, del, r_pair, rinv_pair, radi, radj, vi, tv3(vj4), wi, tv3(wj4), Fp, T);
      }
      v[0] += 0.5 * del.x * Fp.x;
      v[1] += 0.5 * del.y * Fp.y;
      v[2] += 0.5 * del.z * Fp.z;
      v[3] += 0.5 * del.x * Fp.y;
      v[4] += 0.5 * del.x * Fp.z;
      v[5] += 0.5 * del.y * Fp.z;
    }
  }
  block_reduce_store<6, 0>(v, out + 6 * (size_t)blockIdx.x);
}

// FINAL = false: per-block rows of the kinetic tensor and the force norms of the owned atoms.
// FINAL = true (one block): every row of the above and of k_thermo_virial, folded in a fixed order into kResult values.
template <bool FINAL>
__global__ __launch_bounds__(kThermoBlock) void k_thermo_reduce(const double4* vm, const double4* f, int n,
                                                                 const double* kin, int nk, const double* vir, int nv,
                                                                 double* out)
{
  if (!FINAL) {
    double v[kKinRow] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const double4 a = vm[i];
      const double m = a.w;
      v[0] += m * a.x * a.x;
      v[1] += m * a.y * a.y;
      v[2] += m * a.z * a.z;
      v[3] += m * a.x * a.y;
      v[4] += m * a.x * a.z;
      v[5] += m * a.y * a.z;
      const double4 g = f[i];
      v[6] += g.x * g.x + g.y * g.y + g.z * g.z;
      v[7] = fmax(v[7], fmax(fabs(g.x), fmax(fabs(g.y), fabs(g.z))));
    }
    block_reduce_store<kKinRow, 1>(v, out + kKinRow * (size_t)blockIdx.x);
  } else {
    double v[kResult];
#pragma unroll
    for (int c = 0; c < kResult; c++) v[c] = 0.0;
    for (int b = threadIdx.x; b < nk; b += blockDim.x) {
#pragma unroll
      for (int c = 0; c < 7; c++) v[c] += kin[kKinRow * (size_t)b + c];
      v[13] = fmax(v[13], kin[kKinRow * (size_t)b + 7]);
    }
    for (int b = threadIdx.x; b < nv; b += blockDim.x)
#pragma unroll
      for (int c = 0; c < 6; c++) v[7 + c] += vir[6 * (size_t)b + c];
    block_reduce_store<kResult, 1>(v, out);
  }
}

// ---- host side ----

enum Key {
  K_STEP, K_ELAPSED, K_ELAPLONG, K_DT, K_TIME, K_CPU, K_ATOMS, K_TEMP, K_PRESS, K_PE, K_KE, K_ETOTAL, K_EVDWL, K_ECOUL,
  K_EPAIR, K_EMOL, K_VOL, K_LX, K_LY, K_LZ, K_XLO, K_XHI, K_YLO, K_YHI, K_ZLO, K_ZHI, K_PXX, K_PYY, K_PZZ, K_PXY, K_PXZ,
  K_PYZ, K_FMAX, K_FNORM, K_COUNT
};
struct KeyInfo {
  const char* name;     // thermo_style custom keyword
  const char* header;   // [3P] Thermo::addfield names
  bool integer;         // %8ld instead of %12.8g
  bool virial;          // needs the pair virial
};
const KeyInfo kKeys[K_COUNT] = {
    {"step", "Step", true, false},       {"elapsed", "Elapsed", true, false}, {"elaplong", "Elaplong", true, false},
    {"dt", "Dt", false, false},          {"time", "Time", false, false},      {"cpu", "CPU", false, false},
    {"atoms", "Atoms", true, false},     {"temp", "Temp", false, false},      {"press", "Press", false, true},
    {"pe", "PotEng", false, false},      {"ke", "KinEng", false, false},      {"etotal", "TotEng", false, false},
    {"evdwl", "E_vdwl", false, false},   {"ecoul", "E_coul", false, false},   {"epair", "E_pair", false, false},
    {"emol", "E_mol", false, false},     {"vol", "Volume", false, false},     {"lx", "Lx", false, false},
    {"ly", "Ly", false, false},          {"lz", "Lz", false, false},          {"xlo", "Xlo", false, false},
    {"xhi", "Xhi", false, false},        {"ylo", "Ylo", false, false},        {"yhi", "Yhi", false, false},
    {"zlo", "Zlo", false, false},        {"zhi", "Zhi", false, false},        {"pxx", "Pxx", false, true},
    {"pyy", "Pyy", false, true},         {"pzz", "Pzz", false, true},         {"pxy", "Pxy", false, true},
    {"pxz", "Pxz", false, true},         {"pyz", "Pyz", false, true},         {"fmax", "Fmax", false, false},
    {"fnorm", "Fnorm", false, false},
};
const std::vector<int> kStyleOne = {K_STEP, K_TEMP, K_EPAIR, K_EMOL, K_ETOTAL, K_PRESS};

struct ComputeCol {   // a c_ID / c_ID[k] column of thermo_style custom: a global compute (sf_global.hip)
  std::string word, id;
  long index = 0;
  double value = 0.0;   // as printed in the last line
};

struct Thermo {
  // settings
  long long every = 0;                          // `thermo N` (LAMMPS default 0)
  std::vector<int> keys = kStyleOne;            // < K_COUNT: a row of kKeys; K_COUNT + j: ccols[j]
  std::vector<ComputeCol> ccols;
  bool norm_user = false, norm_value = false;   // thermo_modify norm (unset: by units)
  bool flush = false;
  bool lj = true;                               // units lj | si
  // destinations: *_named on every rank (what the script / argv asked for), the FILE* on the writing rank only
  bool screen_named = false, log_named = false;
  FILE* screen = nullptr;
  bool screen_own = false;
  FILE* log = nullptr;
  bool echo_screen = false, echo_log = true;    // [3P] Input: `echo log` by default
  // the run
  long long run_first = 0, run_last = 0, last_line = -1;
  int run_n = 0;
  std::chrono::steady_clock::time_point t_loop;
  bool in_loop = false;
  long long vlaunch_mark = -1;                  // the engine's virial launches when the pass was armed (-1: not armed)
  // `time` ([3P] Update::atime / atimestep)
  double atime = 0.0;
  long long atimestep = 0;
  // device
  double* d_rows = nullptr;                     // [kReduceMaxBlocks][kKinRow], then kResult
  double* h_res = nullptr;                      // pinned [kResult]
  long long launches = 0;
  // last values
  double vir[6] = {0, 0, 0, 0, 0, 0};           // the virial tallied last (all ranks)
  double val[K_COUNT] = {};
  bool have_line = false;

  ~Thermo()
  {
    if (log) fclose(log);
    if (screen && screen_own) fclose(screen);
    else if (screen) fflush(screen);
    if (d_rows) (void)hipFree(d_rows);
    if (h_res) (void)hipHostFree(h_res);
  }
  bool norm() const { return norm_user ? norm_value : lj; }
  bool needs_virial() const
  {
    for (int k : keys)
      if (k < K_COUNT && kKeys[k].virial) return true;
    return false;
  }
};

Thermo* get(const SfLammps& L) { return L.thermo.get<Thermo>(); }
Thermo& ensure(SfLammps& L) { return L.thermo.ensure<Thermo>(); }

// only rank 0 writes (a host that decomposed through sf_slab_init keeps world_rank 0 on every rank: its engine rank counts)
bool writer(const SfLammps& L) { return L.world_rank == 0 && L.eng.rank() == 0; }

void set_screen(SfLammps& L, Thermo& T, const std::string& v)
{
  if (T.screen && T.screen_own) fclose(T.screen);
  T.screen = nullptr;
  T.screen_own = false;
  T.screen_named = v != "none";
  if (!T.screen_named || !writer(L)) return;
  if (v == "stdout") {
    T.screen = stdout;
  } else {
    T.screen = fopen(v.c_str(), "w");
    if (!T.screen) fail("Cannot open screen file %s", v.c_str());
    T.screen_own = true;
  }
}

void set_log(SfLammps& L, Thermo& T, const std::string& v, bool append)
{
  if (T.log) fclose(T.log);
  T.log = nullptr;
  T.log_named = v != "none";
  if (!T.log_named || !writer(L)) return;
  T.log = fopen(v.c_str(), append ? "a" : "w");
  if (!T.log) fail("Cannot open logfile %s", v.c_str());
}

void out(const SfLammps& L, Thermo& T, const char* s)
{
  if (!writer(L)) return;   // (the engine rank of a host that decomposed after opening)
  if (T.screen) fputs(s, T.screen);
  if (T.log) fputs(s, T.log);
  if (T.flush) {
    if (T.screen) fflush(T.screen);
    if (T.log) fflush(T.log);
  }
}

void header(const SfLammps& L, Thermo& T)
{
  std::string h;
  for (int k : T.keys) {
    h += k < K_COUNT ? std::string(kKeys[k].header) : T.ccols[k - K_COUNT].word;   // ([3P] a compute column: the word as typed)
    h += ' ';
  }
  h += '\n';
  out(L, T, h.c_str());
}

// the whole-bed sums on the device, combined over the ranks: K[6] = sum m v_a v_b, f2, fmax, natoms -- and T.vir when
// the virial pass ran for this step
void reduce(SfLammps& L, Thermo& T, double K[6], double* f2, double* fmax, double* natoms)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  if (!T.d_rows) {
    SF_HIP(hipMalloc(&T.d_rows, sizeof(double) * (kReduceMaxBlocks * kKinRow + kResult)));
    SF_HIP(hipHostMalloc(&T.h_res, sizeof(double) * kResult));
  }
  const bool fresh = T.vlaunch_mark >= 0 && e.thermo_virial_launches() > T.vlaunch_mark;
  T.vlaunch_mark = -1;
  const int n = e.nlocal();
  const int nk = std::min(kReduceMaxBlocks, std::max(1, div_up(n, kThermoBlock)));
  const int nv = fresh ? e.thermo_virial_blocks() : 0;
  double* res = T.d_rows + kReduceMaxBlocks * kKinRow;
  k_thermo_reduce<false><<<nk, kThermoBlock, 0, st>>>(e.d_vm(), e.d_force(), n, nullptr, 0, nullptr, 0, T.d_rows);
  k_thermo_reduce<true><<<1, kThermoBlock, 0, st>>>(nullptr, nullptr, 0, T.d_rows, nk, e.thermo_virial_partials(), nv,
                                                    res);
  SF_HIP(hipGetLastError());
  T.launches += 2;
  SF_HIP(hipMemcpyAsync(T.h_res, res, sizeof(double) * kResult, hipMemcpyDeviceToHost, st));
  SF_HIP(hipStreamSynchronize(st));
  // over the ranks: 13 sums and the atom count, then one slot per rank for the maximum (each slot holds one rank's value)
  const int W = std::max(std::max(L.world_size, e.nranks()), 1);
  std::vector<double> buf(14 + W, 0.0);
  for (int c = 0; c < 13; c++) buf[c] = T.h_res[c];
  buf[13] = (double)n;
  const int me = L.world_size > 1 ? L.world_rank : e.rank();
  buf[14 + me] = T.h_res[13];
  if (sf_slab_active(&L) == 1 && sf_slab_allreduce_sum(&L, buf.data(), (int)buf.size()) != 0)
    fail("%s", last_error().c_str());
  for (int c = 0; c < 6; c++) K[c] = buf[c];
  *f2 = buf[6];
  if (fresh)
    for (int c = 0; c < 6; c++) T.vir[c] = buf[7 + c];
  *natoms = buf[13];
  double m = 0.0;
  for (int r = 0; r < W; r++) m = std::max(m, buf[14 + r]);
  *fmax = m;
}

// the c_ columns against the computes as they stand ([3P] Thermo::parse_fields wording); at the thermo_style line and at
// every line (a compute may have been removed since)
void check_compute_cols(const SfLammps& L, const std::vector<ComputeCol>& cols)
{
  if (cols.empty()) return;
  if (L.world_size > 1 || L.decomposed || L.eng.nranks() > 1 || L.eng.decomposed())
    fail("thermo_style custom: c_ columns on one rank only (no decomposed domain)");
  for (const ComputeCol& c : cols) fail_if(check_thermo(compute_shape(L, c.id), c.index, c.id));
}

void line(SfLammps& L, Thermo& T)
{
  DemEngine& e = L.eng;
  double K[6], f2, fmax, N;
  reduce(L, T, K, &f2, &fmax, &N);
  const long long step = e.nsteps();
  double lo[3], hi[3];
  int per[3];
  e.box(lo, hi, per);
  const double lx = hi[0] - lo[0], ly = hi[1] - lo[1], lz = hi[2] - lo[2], V = lx * ly * lz;
  const double boltz = T.lj ? 1.0 : 1.3806504e-23;   // [3P] Force: mvv2e = nktv2p = 1 in both
  const double mv2 = K[0] + K[1] + K[2];
  const double dof = 3.0 * N - 3.0;
  const double temp = dof > 0.0 ? mv2 / (dof * boltz) : 0.0;
  const double nrm = (T.norm() && N > 0.0) ? 1.0 / N : 1.0;
  const double* W = T.vir;
  double* v = T.val;
  v[K_STEP] = (double)step;
  v[K_ELAPSED] = v[K_ELAPLONG] = (double)(step - T.run_first);
  v[K_DT] = e.timestep();
  v[K_TIME] = T.atime + (double)(step - T.atimestep) * e.timestep();
  v[K_CPU] = T.in_loop ? std::chrono::duration<double>(std::chrono::steady_clock::now() - T.t_loop).count() : 0.0;
  v[K_ATOMS] = N;
  v[K_TEMP] = temp;
  v[K_PRESS] = (mv2 + W[0] + W[1] + W[2]) / (3.0 * V);
  v[K_PE] = v[K_EVDWL] = v[K_ECOUL] = v[K_EPAIR] = v[K_EMOL] = 0.0;
  v[K_KE] = 0.5 * mv2 * nrm;
  v[K_ETOTAL] = v[K_KE] + v[K_PE];
  v[K_VOL] = V;
  v[K_LX] = lx;
  v[K_LY] = ly;
  v[K_LZ] = lz;
  v[K_XLO] = lo[0];
  v[K_XHI] = hi[0];
  v[K_YLO] = lo[1];
  v[K_YHI] = hi[1];
  v[K_ZLO] = lo[2];
  v[K_ZHI] = hi[2];
  for (int c = 0; c < 6; c++) v[K_PXX + c] = (K[c] + W[c]) / V;
  v[K_FMAX] = fmax;
  v[K_FNORM] = std::sqrt(f2);
  if (!T.ccols.empty()) {
    // the columns of one compute share one copy; extensive values / natoms under norm yes ([3P] Thermo::compute_compute)
    check_compute_cols(L, T.ccols);
    std::vector<double> vals;
    for (size_t j = 0; j < T.ccols.size(); j++) {
      ComputeCol& cc = T.ccols[j];
      if (j == 0 || T.ccols[j - 1].id != cc.id) global_values_host(L, cc.id, &vals);
      cc.value = vals[cc.index > 0 ? cc.index - 1 : 0];
      if (global_compute_extensive(L, cc.id) && T.norm() && N > 0.0) cc.value /= N;
    }
  }
  T.have_line = true;
  T.last_line = step;
  std::string s;
  char b[64];
  for (int k : T.keys) {
    if (k >= K_COUNT) snprintf(b, sizeof(b), "%12.8g ", T.ccols[k - K_COUNT].value);
    else if (kKeys[k].integer) snprintf(b, sizeof(b), "%8ld ", (long)v[k]);
    else snprintf(b, sizeof(b), "%12.8g ", v[k]);
    s += b;
  }
  s += '\n';
  out(L, T, s.c_str());
}

bool yes_no(const std::string& s)
{
  if (s == "yes") return true;
  if (s == "no") return false;
  fail("Illegal thermo_modify command");
  return false;
}

void refuse_ghost_slots(SfLammps& L)
{
  if (sf_slab_direct_halo(&L) == 2)
    fail("thermo: the pressure keywords are not available with the ghost-slot transport (SF_HALO_DIRECT=2)");
}

}  // namespace

// ---- the virial pass behind DemEngine::launch_substep ----

int thermo_virial_blocks(int nlocal) { return std::min(kVirialMaxBlocks, std::max(1, div_up(nlocal, kThermoBlock))); }

void thermo_virial_launch(const DemPtrs& P, const StepParams& S, bool lub, double* out, int nblocks, hipStream_t st)
{
  const dim3 g(nblocks), b(kThermoBlock);
  style_dispatch(S.gran.style, [&](auto style) {
    flag_dispatch(lub, [&](auto l) { k_thermo_virial<style, l><<<g, b, 0, st>>>(P, S, out); });
  });
  SF_HIP(hipGetLastError());
}

// ---- script surface ----

void thermo_open_args(SfLammps& L, int argc, char** argv)
{
  std::string scr, lg;
  bool have_scr = false, have_log = false;
  for (int k = 1; argv && k < argc; k++) {   // ([3P] LAMMPS::LAMMPS: argv[0] is the program)
    if (!argv[k]) continue;
    const std::string a = argv[k];
    const bool is_scr = a == "-screen" || a == "-sc", is_log = a == "-log" || a == "-l";
    if (!is_scr && !is_log) continue;
    if (k + 1 >= argc || !argv[k + 1]) fail("Invalid command-line argument");
    (is_scr ? scr : lg) = argv[++k];
    (is_scr ? have_scr : have_log) = true;
  }
  // hosts that pass argv = NULL (the reference's softParticleCloud.C): the same through the environment
  if (!have_scr)
    if (const char* v = env_str("SF_SCREEN")) have_scr = !(scr = v).empty();
  if (!have_log)
    if (const char* v = env_str("SF_LOG")) have_log = !(lg = v).empty();
  if (!have_scr && !have_log) return;   // (the default: none and none)
  Thermo& T = ensure(L);
  if (have_scr) set_screen(L, T, scr);
  if (have_log) set_log(L, T, lg, false);
}

void thermo_echo(SfLammps& L, const std::string& text)
{
  Thermo* T = get(L);
  if (!T || (!T->screen && !T->log) || !writer(L)) return;
  std::string s = text;
  while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
  s += '\n';
  if (T->echo_screen && T->screen) fputs(s.c_str(), T->screen);
  if (T->echo_log && T->log) fputs(s.c_str(), T->log);
}

void thermo_units(SfLammps& L, bool lj)
{
  if (!lj || L.thermo) ensure(L).lj = lj;
}

bool thermo_units_lj(const SfLammps& L)
{
  const Thermo* T = get(L);
  return T ? T->lj : true;
}

void thermo_update_time(SfLammps& L)
{
  // [3P] Update::update_time, what the timestep command does before dt changes (lammps_set_timestep does not)
  Thermo& T = ensure(L);
  const long long step = L.eng.nsteps();
  T.atime += (double)(step - T.atimestep) * L.eng.timestep();
  T.atimestep = step;
}

bool thermo_command(SfLammps& L, const std::vector<std::string>& w)
{
  const std::string& c = w[0];
  if (c == "thermo") {
    if (w.size() != 2) fail("Illegal thermo command");
    char* end = nullptr;
    const long long n = std::strtoll(w[1].c_str(), &end, 10);
    if (end == w[1].c_str() || *end || n < 0) fail("Illegal thermo command");
    ensure(L).every = n;
  } else if (c == "thermo_style") {
    if (w.size() < 2) fail("Illegal thermo_style command");
    std::vector<int> keys;
    std::vector<ComputeCol> ccols;
    if (w[1] == "one") {
      if (w.size() != 2) fail("Illegal thermo_style command");
      keys = kStyleOne;
    } else if (w[1] == "multi") {
      fail("thermo_style multi is not supported by this engine (one and custom are)");
    } else if (w[1] == "custom") {
      if (w.size() < 3) fail("Illegal thermo_style command");
      for (size_t a = 2; a < w.size(); a++) {
        int k = 0;
        while (k < K_COUNT && w[a] != kKeys[k].name) k++;
        if (k == K_COUNT && w[a].compare(0, 2, "c_") == 0) {   // a global compute
          ComputeCol cc;
          cc.word = w[a];
          const std::string err = parse_thermo_column(w[a], &cc.id, &cc.index);
          if (!err.empty()) fail("%s", err.c_str());
          k = K_COUNT + (int)ccols.size();
          ccols.push_back(cc);
        } else if (k == K_COUNT)
          fail("Invalid keyword in thermo_style custom command: %s", w[a].c_str());
        keys.push_back(k);
      }
      check_compute_cols(L, ccols);
    } else {
      fail("Illegal thermo_style command: style %s", w[1].c_str());
    }
    Thermo& T = ensure(L);
    T.keys = keys;
    T.ccols = ccols;
    T.norm_user = false;   // [3P] a new Thermo: norm and flush back to their defaults
    T.flush = false;
  } else if (c == "thermo_modify") {
    if (w.size() < 3) fail("Illegal thermo_modify command");
    Thermo& T = ensure(L);
    for (size_t a = 1; a < w.size(); a += 2) {
      const std::string& k = w[a];
      if (k != "norm" && k != "flush" && k != "lost")
        fail("thermo_modify %s is not supported by this engine (norm, flush and lost error are)", k.c_str());
      if (a + 1 >= w.size()) fail("Illegal thermo_modify command");
      const std::string& v = w[a + 1];
      if (k == "norm") {
        T.norm_user = true;
        T.norm_value = yes_no(v);
      } else if (k == "flush") {
        T.flush = yes_no(v);
      } else if (k == "lost") {
        if (v != "error")
          fail("thermo_modify lost %s is not supported: this engine always stops on a lost atom (lost error)", v.c_str());
      }
    }
  } else if (c == "log") {
    if (w.size() < 2 || w.size() > 3 || (w.size() == 3 && w[2] != "append")) fail("Illegal log command");
    set_log(L, ensure(L), w[1], w.size() == 3);
  } else if (c == "echo") {
    if (w.size() != 2) fail("Illegal echo command");
    Thermo& T = ensure(L);
    if (w[1] == "none" || w[1] == "screen" || w[1] == "log" || w[1] == "both") {
      T.echo_screen = w[1] == "screen" || w[1] == "both";
      T.echo_log = w[1] == "log" || w[1] == "both";
    } else {
      fail("Illegal echo command");
    }
  } else {
    return false;
  }
  return true;
}

// ---- the run ----

bool thermo_active(const SfLammps& L)
{
  const Thermo* T = get(L);
  return T && (T->screen_named || T->log_named);
}

bool thermo_needs_dof(const SfLammps& L)
{
  const Thermo* T = get(L);
  if (!T) return false;
  for (int k : T->keys)
    if (k == K_TEMP || k == K_PRESS || k == K_KE || k == K_ETOTAL || (k < K_COUNT && kKeys[k].virial)) return true;
  return false;
}

void thermo_run_begin(SfLammps& L)
{
  Thermo& T = *get(L);
  L.eng.set_thermo_virial(false);
  T.vlaunch_mark = -1;
  // the first run's setup evaluates the forces (mode 2): the setup line shows that evaluation's virial; the setup of a
  // later run evaluates nothing and shows the virial tallied last, as LAMMPS' does after `pre no`
  if (!L.eng.is_setup() && T.needs_virial()) {
    refuse_ghost_slots(L);
    T.vlaunch_mark = L.eng.thermo_virial_launches();
    L.eng.set_thermo_virial(true);
  }
}

void thermo_setup(SfLammps& L, int n)
{
  Thermo& T = *get(L);
  L.eng.set_thermo_virial(false);
  T.run_first = L.eng.nsteps();
  T.run_n = n > 0 ? n : 0;
  T.run_last = T.run_first + T.run_n;
  T.in_loop = false;
  header(L, T);
  line(L, T);
  T.t_loop = std::chrono::steady_clock::now();
  T.in_loop = true;
}

long long thermo_next_step(const SfLammps& L, long long step)
{
  const Thermo& T = *get(L);
  long long next = T.run_last;
  if (T.every > 0) next = std::min(next, (step / T.every + 1) * T.every);
  return next;
}

void thermo_arm(SfLammps& L, long long end)
{
  Thermo& T = *get(L);
  const bool on = (end == T.run_last || (T.every > 0 && end % T.every == 0)) && T.needs_virial();
  if (on) refuse_ghost_slots(L);
  T.vlaunch_mark = on ? L.eng.thermo_virial_launches() : -1;
  L.eng.set_thermo_virial(on);
}

void thermo_write_due(SfLammps& L)
{
  Thermo& T = *get(L);
  L.eng.set_thermo_virial(false);
  const long long step = L.eng.nsteps();
  if (step == T.last_line) return;
  if (step == T.run_last || (T.every > 0 && step % T.every == 0)) line(L, T);
}

void thermo_run_end(SfLammps& L)
{
  Thermo& T = *get(L);
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - T.t_loop).count();
  T.in_loop = false;
  T.last_line = -1;
  char b[256];
  const int procs = std::max(std::max(L.world_size, L.eng.nranks()), 1);
  snprintf(b, sizeof(b), "Loop time of %g on %d procs for %d steps with %lld atoms\n\n", secs, procs, T.run_n,
           (long long)T.val[K_ATOMS]);
  out(L, T, b);
  if (T.screen) fflush(T.screen);
  if (T.log) fflush(T.log);
}

std::vector<std::string> thermo_global_ids_due(const SfLammps& L, bool setup, int run_n)
{
  std::vector<std::string> ids;
  const Thermo* T = get(L);
  if (!T || T->ccols.empty() || !thermo_active(L)) return ids;
  const long long step = L.eng.nsteps();
  const long long last = setup ? step + (run_n > 0 ? run_n : 0) : T->run_last;
  if (!setup && (step == T->last_line || !(step == last || (T->every > 0 && step % T->every == 0)))) return ids;
  for (const ComputeCol& c : T->ccols)
    if (std::find(ids.begin(), ids.end(), c.id) == ids.end()) ids.push_back(c.id);
  return ids;
}

bool thermo_uses_compute(const SfLammps& L, const std::string& id)
{
  const Thermo* T = get(L);
  if (!T) return false;
  for (const ComputeCol& c : T->ccols)
    if (c.id == id) return true;
  return false;
}

int thermo_get(const SfLammps& L, const std::string& keyword, double* v)
{
  if (keyword.compare(0, 2, "c_") == 0) {   // a compute column of the current style, by the word as typed
    const Thermo* T = get(L);
    if (T)
      for (const ComputeCol& c : T->ccols)
        if (c.word == keyword) {
          if (!T->have_line) return -1;
          *v = c.value;
          return 0;
        }
    return -2;
  }
  int k = 0;
  while (k < K_COUNT && keyword != kKeys[k].name) k++;
  if (k == K_COUNT) return -2;
  const Thermo* T = get(L);
  if (!T || !T->have_line) return -1;
  *v = T->val[k];
  return 0;
}

long long thermo_launches(const SfLammps& L)
{
  const Thermo* T = get(L);
  return L.eng.thermo_virial_launches() + (T ? T->launches : 0);
}

}  // namespace sf
