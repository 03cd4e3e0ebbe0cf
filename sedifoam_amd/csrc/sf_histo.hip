// sf_histo.hip -- fix ave/histo ([3P] LAMMPS names, rules and wording):
//   fix ID group ave/histo Nevery Nrepeat Nfreq lo hi Nbin value ... [mode scalar|vector] [kind global|peratom|local]
//       [beyond ignore|end|extra] [ave one|running|window M] [start N] [file F] [overwrite] [title1|title2|title3 S]
//   values: x y z vx vy vz fx fy fz and c_ID / c_ID[k] of a per-atom compute (over the atoms of the group), c_ID / c_ID[k] of
//   a compute pair/local (over all of its rows), c_ID / c_ID[k] of a global compute; all of one kind, all into one histogram
// A sample counts the state AT THE MOMENT OF THE SAMPLE, like a dump frame, and stores nothing back into the run.
//
// One sample, on the engine's stream:
//   k_histo_bin  a by-value table of the fix's value columns (the descriptor and loader of sf_gather_col.h).  Block-stride
//                over the elements with a grid that depends on the element count alone; a record several columns need is
//                loaded once.  Each lane computes the bin of its value with histo_bin (sf_histo_parse.h, the expression the
//                host and the NumPy model evaluate); the block counts in a 32-bit histogram in LDS with LDS integer atomics
//                -- one ballot per column finds the wave whose lanes all share one bin (a bed at rest), where one lane adds
//                the population count -- and then adds its non-zero bins, total and missing into the fix's 64-bit device
//                counters with integer atomics.  min and max go through an order-preserving integer image of the double
//                and an integer atomic max.
// Integer adds and maxima are exact in any order: the same state gives the same bits.  No floating-point atomics, no
// scratch.  The counters stay on the device over the Nrepeat samples of an output; a sample that is not an output copies
// nothing to the host and waits for nothing (but for the row count that contact_rows reads for local inputs).  At an output
// the counters are copied once to pinned memory and zeroed on the stream.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_ave_fix.h"
#include "sf_compute_atom.h"
#include "sf_compute_ids.h"
#include "sf_contacts.h"
#include "sf_gather_col.h"
#include "sf_global.h"
#include "sf_histo.h"

// ((v - lo) * bininv stays a difference and a product, whatever the compiler would fuse around it: the bin of a value is
// the integer the host computes)
#pragma clang fp contract(off)
#include "sf_histo_parse.h"

namespace sf {
namespace {

constexpr int kHBlock = 256;
constexpr int kHMaxBlocks = 1024;
constexpr int kHExtra = 4;   // behind the nbins counters of a fix: total, missing, the images of min and of max

struct HTable {
  int n;
  unsigned need;
  GCol c[kHistoMaxValues];
  int lim[kHistoMaxValues];   // global inputs: the elements of this column (0: every element of the launch)
};

// the order of the doubles as an order of unsigned integers (-0.0 below +0.0); 0 is the image of no double that a
// comparison can produce (a negative NaN of all ones), so zeroed counters mean "no value yet"
__host__ __device__ inline unsigned long long histo_key(double v)
{
  unsigned long long u;
  memcpy(&u, &v, sizeof(u));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
double histo_unkey(unsigned long long k)
{
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &u, sizeof(v));
  return v;
}

// acc: [nbins] counts, total, missing, ~key(min), key(max).  Dynamic LDS: (nbins + 2) counters of 32 bits -- a block
// visits at most ceil(n / gridDim) elements of at most 16 columns, below 2^32 for every n below 2^37
__global__ __launch_bounds__(kHBlock) void k_histo_bin(GRecords R, HTable T, HistoBins B, long long n, unsigned long long* acc)
{
  extern __shared__ unsigned int h[];
  __shared__ double wmn[kHBlock / 64], wmx[kHBlock / 64];
  const int nb2 = B.nbins + 2;
  for (int b = threadIdx.x; b < nb2; b += kHBlock) h[b] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  double mn = 1.0e20, mx = -1.0e20;
  unsigned int total = 0u, missing = 0u;
  const long long stride = (long long)gridDim.x * kHBlock;
  // (every lane of the block stays in the loop, so that the ballots below see whole waves)
  for (long long base = (long long)blockIdx.x * kHBlock; base < n; base += stride) {
    const long long i = base + threadIdx.x;
    const bool valid = i < n;
    const double4 zero = make_double4(0.0, 0.0, 0.0, 0.0);
    double4 xr = zero, vm = zero, f = zero;
    int mask = 0;
    if (valid) {
      if (T.need & GN_XR) xr = R.xr[i];
      if (T.need & GN_VM) vm = R.vm[i];
      if (T.need & GN_FORCE) f = R.force[i];
      if (T.need & GN_MASK) mask = R.mask[i];
    }
#pragma unroll
    for (int q = 0; q < kHistoMaxValues; q++) {
      if (q < T.n) {
        const GCol c = T.c[q];
        const int lim = T.lim[q];
        const bool on = valid && (c.groupbit == 0 || (mask & c.groupbit)) && (lim == 0 || i < (long long)lim);
        int bin = -1;
        if (on) {
          const double v = g_value(c, i, xr, vm, zero, f, zero);
          mn = fmin(mn, v);
          mx = fmax(mx, v);
          bin = histo_bin(B, v);
          if (bin < 0) missing++;
          else total++;
        }
        const bool counted = bin >= 0;
        const unsigned long long m = __ballot(counted);
        if (m) {
          const int first = __ffsll((long long)m) - 1;
          const int b0 = __shfl(bin, first, 64);
          if (__ballot(counted && bin != b0) == 0ull) {   // the one-bin wave: 64 lanes would hit one LDS address
            if (lane == first) atomicAdd(&h[b0], (unsigned int)__popcll(m));
          } else if (counted)
            atomicAdd(&h[bin], 1u);
        }
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    total += __shfl_down(total, off, 64);
    missing += __shfl_down(missing, off, 64);
    mn = fmin(mn, __shfl_down(mn, off, 64));
    mx = fmax(mx, __shfl_down(mx, off, 64));
  }
  if (lane == 0) {
    if (total) atomicAdd(&h[B.nbins], total);
    if (missing) atomicAdd(&h[B.nbins + 1], missing);
    wmn[threadIdx.x >> 6] = mn;
    wmx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb2; b += kHBlock) {
    const unsigned int k = h[b];
    if (k) atomicAdd(&acc[b], (unsigned long long)k);
  }
  if (threadIdx.x == 0) {
    for (int w = 1; w < kHBlock / 64; w++) {
      mn = fmin(mn, wmn[w]);
      mx = fmax(mx, wmx[w]);
    }
    atomicMax(&acc[nb2], ~histo_key(mn));
    atomicMax(&acc[nb2 + 1], histo_key(mx));
  }
}

// ---- host side ----

struct HistoFix : AveFixState {
  HistoSpec S;
  HistoBins B;
  int kind = HK_PERATOM;
  int groupbit = 1;
  unsigned long long* acc = nullptr;   // device [nbins + kHExtra]
  HistoAverager A;
  HistoBlock out;   // the latest output
  size_t nacc() const { return (size_t)B.nbins + kHExtra; }
  ~HistoFix()
  {
    if (acc) (void)hipFree(acc);
  }
};

struct HistoSet {
  std::vector<std::unique_ptr<HistoFix>> fixes;
  unsigned long long* h_buf = nullptr;      // pinned [kHistoMaxBins + 2 + kHExtra]
  unsigned long long* cost_acc = nullptr;   // device, the same size: where sf_lammps_ave_histo_cost counts
  long long launches = 0, host_copies = 0;
  static constexpr size_t kMaxAcc = (size_t)kHistoMaxBins + 2 + kHExtra;
  ~HistoSet()
  {
    if (h_buf) (void)hipHostFree(h_buf);
    if (cost_acc) (void)hipFree(cost_acc);
  }
  HistoFix* find_fix(const std::string& id) const { return ave_find(fixes, id); }
  void device()
  {
    if (h_buf) return;
    SF_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_buf), sizeof(unsigned long long) * kMaxAcc));
    SF_HIP(hipMalloc(&cost_acc, sizeof(unsigned long long) * kMaxAcc));
  }
};

HistoSet* set_of(const SfLammps& L) { return L.histos.get<HistoSet>(); }
HistoSet& ensure_set(SfLammps& L) { return L.histos.ensure<HistoSet>(); }

// The kind of the values and every rule that needs the computes: checked at the fix line and again at every sample (a
// compute may have been removed and defined anew)
int check_values(const SfLammps& L, const HistoSpec& S)
{
  std::vector<int> kinds;
  for (const HistoValue& v : S.values) {
    if (v.attr != AA_COMPUTE) {
      kinds.push_back(HK_PERATOM);
      continue;
    }
    const ComputeShape shape = compute_shape(L, v.id);
    fail_if(check_ave_histo_kind(shape, v.id));
    kinds.push_back(shape.kind == CK_PERATOM ? HK_PERATOM : (shape.kind == CK_LOCAL ? HK_LOCAL : HK_GLOBAL));
  }
  const int kind = kinds[0];
  for (int k : kinds)
    if (k != kind) fail("Fix ave/histo inputs are not all global, peratom, or local");
  static const char* const names[3] = {"global", "peratom", "local"};
  if (S.kind != HK_NONE && S.kind != kind)
    fail("fix ave/histo: kind %s does not agree with the values, which are %s", names[S.kind], names[kind]);
  if (kind == HK_PERATOM && S.mode == HM_SCALAR) fail("Fix ave/histo cannot input per-atom values in scalar mode");
  if (kind == HK_LOCAL && S.mode == HM_SCALAR) fail("Fix ave/histo cannot input local values in scalar mode");
  for (const HistoValue& v : S.values)
    if (v.attr == AA_COMPUTE) fail_if(check_ave_histo_index(compute_shape(L, v.id), v.index, S.mode == HM_SCALAR));
  return kind;
}

// The launches of one sample: one table over the atoms, or over the values of the global computes; for local inputs one
// table per compute pair/local that the values name (their row counts differ, and the rows of one compute are valid only
// until the next is evaluated)
std::vector<std::vector<int>> launch_groups(const HistoFix& F)
{
  std::vector<std::vector<int>> groups;
  const int nv = (int)F.S.values.size();
  if (F.kind != HK_LOCAL) {
    groups.emplace_back();
    for (int j = 0; j < nv; j++) groups[0].push_back(j);
    return groups;
  }
  std::vector<std::string> ids;
  for (int j = 0; j < nv; j++) {
    size_t g = 0;
    while (g < ids.size() && ids[g] != F.S.values[j].id) g++;
    if (g == ids.size()) {
      ids.push_back(F.S.values[j].id);
      groups.emplace_back();
    }
    groups[g].push_back(j);
  }
  return groups;
}

// the table of the values `which` of the fix and its element count; evaluates what the columns read (per-atom computes,
// contact rows, global computes) where that is stale
long long build_table(SfLammps& L, const HistoFix& F, const std::vector<int>& which, HTable* T)
{
  DemEngine& e = L.eng;
  *T = HTable{};
  long long n = 0;
  ContactRows rows;
  std::vector<unsigned char> row_values;
  if (F.kind == HK_PERATOM) n = e.nlocal();
  else if (F.kind == HK_LOCAL) {
    int groupbit = 1;
    compute_lookup(L, F.S.values[which[0]].id, &row_values, &groupbit);
    rows = contact_rows(L, groupbit);   // (reads the row count on the host: one wait)
    n = rows.n;
  }
  for (int j : which) {
    const HistoValue& v = F.S.values[j];
    const long col = v.index > 0 ? v.index - 1 : 0;
    GCol c = make_col(nullptr, GS_ZERO, 0, 0, 0);
    int lim = 0;
    if (F.kind == HK_PERATOM) {
      c.groupbit = F.groupbit;
      if (v.attr != AA_COMPUTE) c.set(v.attr < AA_VX ? GS_XR : (v.attr < AA_FX ? GS_VM : GS_FORCE), v.attr % 3, 0);
      else {
        int nc = 0;
        const double* val = atom_compute_values(L, v.id, &nc);   // (once per step however many ask)
        if (val && col < nc) {
          c.set(GS_PTR, 0, 0);
          c.p = val + (size_t)col * (size_t)n;
        }
      }
    } else if (F.kind == HK_LOCAL) {
      const int rv = col < (long)row_values.size() ? row_values[col] : CV_ENG;
      if (rv < kContactDoubles && rows.val) {
        c.set(GS_PTR, 0, 0);
        c.p = rows.val + (size_t)rv * (size_t)rows.n;
      } else if ((rv == CV_TAG1 || rv == CV_TAG2) && rows.tag1 && rows.tag2) {
        c.set(GS_INT, 0, 0);
        c.p = rv == CV_TAG1 ? rows.tag1 : rows.tag2;
      }   // (eng: 0)
    } else {
      const int len = compute_shape(L, v.id).n;
      const double* val = global_values_device(L, v.id);   // (fresh when global_step_due has run at this step)
      c.set(GS_PTR, 0, 0);
      if (F.S.mode == HM_SCALAR) {
        c.p = val + (col < len ? col : 0);
        lim = 1;
      } else {
        c.p = val;
        lim = len;
      }
      n = std::max<long long>(n, lim);
    }
    T->c[T->n] = c;
    T->lim[T->n] = lim;
    T->need |= need_of(c);
    T->n++;
  }
  return n;
}

void launch_table(SfLammps& L, HistoSet& H, const HistoFix& F, const HTable& T, long long n, unsigned long long* acc)
{
  if (n <= 0 || T.n == 0) return;
  DemEngine& e = L.eng;
  const int nb = (int)std::min<long long>(kHMaxBlocks, (n + kHBlock - 1) / kHBlock);
  GRecords R{e.d_xr(), e.d_vm(), e.d_om(), e.d_force(), e.d_torque(), e.d_mask()};
  const size_t lds = sizeof(unsigned int) * ((size_t)F.B.nbins + 2);
  k_histo_bin<<<nb, kHBlock, lds, e.stream()>>>(R, T, F.B, n, acc);
  SF_HIP(hipGetLastError());
  H.launches++;
}

void sample(SfLammps& L, HistoSet& H, HistoFix& F)
{
  refuse_decomposed(L, "fix ave/histo");
  F.kind = check_values(L, F.S);
  for (const std::vector<int>& which : launch_groups(F)) {
    HTable T;
    const long long n = build_table(L, F, which, &T);
    launch_table(L, H, F, T, n, F.acc);
  }
}

void write_block(HistoFix& F)
{
  FILE* fp = F.file.fp();
  if (!fp) return;
  fail_if(F.file.begin_block());
  const HistoBlock& o = F.out;
  fprintf(fp, "%lld %d %g %g %g %g\n", F.out_step, F.B.nbins, o.total, o.missing, o.min, o.max);
  for (int i = 0; i < F.B.nbins; i++) {
    if (o.total > 0.0) fprintf(fp, "%d %g %g %g\n", i + 1, histo_coord(F.B, i), o.count[i], o.count[i] / o.total);
    else fprintf(fp, "%d %g 0 0\n", i + 1, histo_coord(F.B, i));
  }
  fail_if(F.file.end_block());
}

// the counters of Nrepeat samples -> one output: one copy to pinned memory, zeroed on the stream, one wait
void make_output(SfLammps& L, HistoSet& H, HistoFix& F)
{
  hipStream_t st = L.eng.stream();
  const size_t bytes = sizeof(unsigned long long) * F.nacc();
  SF_HIP(hipMemcpyAsync(H.h_buf, F.acc, bytes, hipMemcpyDeviceToHost, st));
  SF_HIP(hipMemsetAsync(F.acc, 0, bytes, st));
  SF_HIP(hipStreamSynchronize(st));
  H.host_copies++;
  const int nb = F.B.nbins;
  HistoBlock b;
  b.count.resize(nb);
  for (int i = 0; i < nb; i++) b.count[i] = (double)H.h_buf[i];
  b.total = (double)H.h_buf[nb];
  b.missing = (double)H.h_buf[nb + 1];
  if (H.h_buf[nb + 2]) b.min = std::min(b.min, histo_unkey(~H.h_buf[nb + 2]));
  if (H.h_buf[nb + 3]) b.max = std::max(b.max, histo_unkey(H.h_buf[nb + 3]));
  F.out = F.A.add(b);
  F.out_step = L.eng.nsteps();
  F.have = true;
  write_block(F);
}

// a fix whose sample step has passed without a sample (steps taken outside run_steps) begins a new output, without the
// samples of the one that was under way.  Is a sample of F due at the engine's step?
bool due_now(SfLammps& L, HistoFix& F)
{
  const long long step = L.eng.nsteps();
  if (F.S.catch_up(step)) SF_HIP(hipMemsetAsync(F.acc, 0, sizeof(unsigned long long) * F.nacc(), L.eng.stream()));
  return F.S.due(step);
}

bool fix_exists(const SfLammps& L, const std::string& id)
{
  HistoSet* H = set_of(L);
  return H && H->find_fix(id);
}

bool unfix(SfLammps& L, const std::string& id)
{
  HistoSet* H = set_of(L);
  return H && ave_take(L, H->fixes, id);
}

bool uses_compute(const SfLammps& L, const std::string& id)
{
  const HistoSet* H = set_of(L);
  if (!H) return false;
  for (const auto& f : H->fixes)
    for (const HistoValue& v : f->S.values)
      if (v.attr == AA_COMPUTE && v.id == id) return true;
  return false;
}

long long next_step(const SfLammps& L, long long step)
{
  const HistoSet* H = set_of(L);
  return H ? ave_next(H->fixes, step) : -1;
}

}  // namespace

const AveFixKind& ave_histo_kind()
{
  static const AveFixKind kind = {"fix ave/histo", fix_exists, unfix, uses_compute, next_step};
  return kind;
}

void ave_histo_fix_command(SfLammps& L, const std::string& line)
{
  std::vector<std::string> w;
  const std::string qerr = split_quoted(line, &w);
  if (!qerr.empty()) fail("%s", qerr.c_str());
  auto F = std::make_unique<HistoFix>();
  fail_if(parse_ave_histo(w, &F->S));
  refuse_decomposed(L, "fix ave/histo");
  F->groupbit = L.eng.group_bit(F->S.group);
  HistoSet& H = ensure_set(L);
  if (ave_fix_exists(L, F->S.id))
    fail("fix ave/histo %s: this fix ID is in use (unfix it first)", F->S.id.c_str());
  F->kind = check_values(L, F->S);
  F->B = histo_bins(F->S.lo, F->S.hi, F->S.nbin, F->S.beyond);
  F->A.ave = F->S.ave;
  F->A.window = F->S.window;
  F->S.begin(L.eng.nsteps());
  H.device();
  const std::string titles[3] = {"# Histogrammed data for fix " + F->S.id,
                                 "# TimeStep Number-of-bins Total-counts Missing-counts Min-value Max-value",
                                 "# Bin Coord Count Count/Total"};
  fail_if(F->file.open(F->S, "ave/histo", F->S.id, titles, 3));
  SF_HIP(hipMalloc(&F->acc, sizeof(unsigned long long) * F->nacc()));
  SF_HIP(hipMemsetAsync(F->acc, 0, sizeof(unsigned long long) * F->nacc(), L.eng.stream()));
  H.fixes.push_back(std::move(F));
}

void ave_histo_global_ids_due(SfLammps& L, std::vector<std::string>* ids)
{
  HistoSet* H = set_of(L);
  if (!H) return;
  for (auto& f : H->fixes) {
    if (!due_now(L, *f) || f->kind != HK_GLOBAL) continue;
    refuse_decomposed(L, "fix ave/histo");
    f->kind = check_values(L, f->S);
    if (f->kind != HK_GLOBAL) continue;
    for (const HistoValue& v : f->S.values)
      if (std::find(ids->begin(), ids->end(), v.id) == ids->end()) ids->push_back(v.id);
  }
}

void ave_histo_sample_due(SfLammps& L)
{
  HistoSet* H = set_of(L);
  if (!H) return;
  for (auto& f : H->fixes) {
    if (!due_now(L, *f)) continue;
    sample(L, *H, *f);
    if (f->S.sampled(L.eng.nsteps())) make_output(L, *H, *f);
  }
}

}  // namespace sf

using sf::handle;

namespace {
sf::HistoFix& fix_of(void* ptr, const char* id)
{
  sf::HistoSet* H = sf::set_of(*handle(ptr));
  sf::HistoFix* F = H ? H->find_fix(id) : nullptr;
  if (!F) sf::fail("Could not find fix ave/histo ID %s", id);
  return *F;
}
}  // namespace

extern "C" {

long long sf_lammps_ave_histo(void* ptr, const char* id, long long max, long long* step, double* stats4, double* coord,
                              double* count)
{
  long long n = 0;
  SF_API_BEGIN
  if (!id) sf::fail("sf_lammps_ave_histo: null argument");
  const sf::HistoFix& F = fix_of(ptr, id);
  if (!F.have) sf::fail("fix ave/histo %s has made no output yet (the first one is due at a multiple of Nfreq)", id);
  n = F.B.nbins;
  if (step) *step = F.out_step;
  if (stats4) {
    stats4[0] = F.out.total;
    stats4[1] = F.out.missing;
    stats4[2] = F.out.min;
    stats4[3] = F.out.max;
  }
  if (max > 0 && n <= max) {
    if (!coord || !count) sf::fail("sf_lammps_ave_histo: null argument");
    for (int i = 0; i < F.B.nbins; i++) coord[i] = sf::histo_coord(F.B, i);
    std::copy(F.out.count.begin(), F.out.count.end(), count);
  }
  SF_API_END(n)
}

int sf_lammps_ave_histo_launches(void* ptr, long long* launches, long long* host_copies)
{
  SF_API_BEGIN
  if (!launches) sf::fail("sf_lammps_ave_histo_launches: null argument");
  const sf::HistoSet* H = sf::set_of(*handle(ptr));
  *launches = H ? H->launches : 0;
  if (host_copies) *host_copies = H ? H->host_copies : 0;
  SF_API_END(0)
}

int sf_lammps_ave_histo_cost(void* ptr, const char* id, double* ms)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id || !ms) sf::fail("sf_lammps_ave_histo_cost: null argument");
  sf::HistoFix& F = fix_of(ptr, id);
  sf::HistoSet& H = *sf::set_of(L);
  sf::refuse_decomposed(L, "fix ave/histo");
  F.kind = sf::check_values(L, F.S);
  hipStream_t st = L.eng.stream();
  // (the counts go into a buffer of the set: the fix's counters are untouched.  What the columns read -- per-atom computes,
  // contact rows, global computes -- is evaluated outside the time: each has a cost query of its own)
  SF_HIP(hipMemsetAsync(H.cost_acc, 0, sizeof(unsigned long long) * F.nacc(), st));
  double total = 0.0;
  for (const std::vector<int>& which : sf::launch_groups(F)) {
    sf::HTable T;
    const long long n = sf::build_table(L, F, which, &T);
    total += sf::stream_ms(st, [&] { sf::launch_table(L, H, F, T, n, H.cost_acc); });
  }
  *ms = total;
  SF_API_END(0)
}

}  // extern "C"
