// sf_global.hip -- whole-bed reductions ([3P] LAMMPS names and rules):
//   compute ID group reduce sum|min|max|ave|sumsq|avesq x y z vx vy vz fx fy fz c_ID c_ID[k] ...
//       per-atom inputs over the atoms of the group, the columns of a compute pair/local over all of its rows; one input a
//       global scalar, several a global vector
//   compute ID group ke | erotate/sphere      the group sums of the terms of ke/atom and erotate/sphere/atom (sf_atom_terms.h)
//   compute ID group com                      sum m unmap(x) / sum m over the group ([3P] Group::xcm), three values
//                                             (a mean squared displacement is compute reduce avesq
//                                             over the columns of a compute displace/atom)
//   compute ID group cluster/stats CID        [own] over the group atoms whose value of compute cluster/atom CID is not 0: the
//                                             distinct cluster IDs, the most atoms under one ID, the atoms; three values
//                                             
//   fix ID group ave/time Nevery Nrepeat Nfreq c_ID c_ID[k] ... [ave one|running|window M] [start N] [file F] [overwrite]
//       [format S] [title1 S] [title2 S]       time averages of global values, one line per Nfreq steps
//       ... c_ID[k] ... mode vector [title3 S]   the columns of global arrays of one row count (compute rdf, sf_nbr.hip): a
//                                             device accumulator [rows][values], k_global_col_acc per column and sample,
//                                             one block of `row value ...` lines per Nfreq steps
// A value is evaluated from the state AT THE MOMENT OF THE OUTPUT, like a dump frame, and stores nothing back into the run.
//
// One evaluation, on the engine's stream:
//   k_global_gather  a by-value table of up to 16 columns (a component of a state record, a per-atom buffer, a contact-row
//                    column, a ke / erotate term; a group bit; sum, sum of squares, min or max).  Grid-stride over the
//                    elements with a grid that depends on the element count alone; a record several columns need is loaded
//                    once; the accumulators stay in registers; wave64 shuffle tree, then the four waves through LDS
//                    (sf_block_reduce.h): one partial row per block
//   k_global_fold    one block folds the partial rows in a fixed order, divides ave / avesq by the count (a count column of
//                    the same launch, or the row count), stores the values, and adds them into the accumulators of the fix
//                    ave/time samples due at this step
//   k_global_unwrapped   compute com: ONE launch.  A group atom loads its two records, mask and tag and gathers its image
//                    counts by tag; the sums stay in registers, go through the same wave64 tree and LDS step into one partial row per block, and the block
//                    that arrives last (an integer ticket behind an agent-scope release) folds the rows in row order and
//                    stores the values
//   k_cluster_rows, k_cluster_stats   compute cluster/stats: an integer counter per tag takes one integer atomic add per
//                    atom; then ONE launch counts the rows that are not zero (ballots), their maximum and their sum through the
//                    same tree and the same last-block fold.  Integers only
// More than 16 columns take more launches; atom columns and row columns have different element counts and go in separate
// launches.  No floating-point atomics, no scratch: the same state gives the same bits, and which thread adds which element
// does not depend on the other columns of the launch.  Nothing is copied to the host before an output step, a thermo line
// or a query.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_atom_terms.h"
#include "sf_ave_fix.h"
#include "sf_block_reduce.h"
#include "sf_compute_atom.h"
#include "sf_compute_ids.h"
#include "sf_contacts.h"
#include "sf_displace.h"
#include "sf_displace_parse.h"
#include "sf_gather_col.h"
#include "sf_pchunk.h"
#include "sf_global.h"
#include "sf_global_parse.h"
#include "sf_nbr.h"

// (a*a + s stays a product and a sum, so that a column's bits do not depend on what the compiler fuses around it)
#pragma clang fp contract(off)

namespace sf {
namespace {

constexpr int kGCols = 16;          // columns of one launch
constexpr int kGBlock = 256;
constexpr int kGMaxBlocks = 1024;   // partial rows
constexpr int kGAcc = 24;           // accumulator additions one fold launch carries
constexpr int kPool = 4096;         // device doubles: the values of the computes and the accumulators of the fixes

enum GOp { GO_SUM, GO_SUMSQ, GO_MIN, GO_MAX };

struct GTable {
  int n;
  unsigned need;
  GCol c[kGCols];
};
struct GFold {
  int n;
  int op[kGCols];
  int div[kGCols];      // -1: none; -2: the row count; >= 0: the count column of this launch
  double* out[kGCols];  // nullptr: not stored (a count column)
  int nacc;
  int acc_col[kGAcc];
  double* acc_dst[kGAcc];
};
struct GAccOnly {   // accumulator additions of values that were already evaluated at this step
  int n;
  const double* src[kGAcc];
  double* dst[kGAcc];
};

__device__ __forceinline__ double g_identity(int op) { return op == GO_MIN ? 1.0e20 : (op == GO_MAX ? -1.0e20 : 0.0); }
__device__ __forceinline__ double g_combine(int op, double a, double b)
{
  return op == GO_MIN ? fmin(a, b) : (op == GO_MAX ? fmax(a, b) : a + b);
}

__global__ __launch_bounds__(kGBlock) void k_global_gather(GRecords R, GTable T, long long n, double* partial)
{
  double acc[kGCols];
#pragma unroll
  for (int q = 0; q < kGCols; q++) acc[q] = q < T.n ? g_identity(T.c[q].op()) : 0.0;
  const long long stride = (long long)gridDim.x * kGBlock;
  for (long long i = (long long)blockIdx.x * kGBlock + threadIdx.x; i < n; i += stride) {
    const double4 zero = make_double4(0.0, 0.0, 0.0, 0.0);
    double4 xr = zero, vm = zero, om = zero, f = zero, tq = zero;
    int mask = 0;
    if (T.need & GN_XR) xr = R.xr[i];
    if (T.need & GN_VM) vm = R.vm[i];
    if (T.need & GN_OM) om = R.om[i];
    if (T.need & GN_FORCE) f = R.force[i];
    if (T.need & GN_TORQUE) tq = R.torque[i];
    if (T.need & GN_MASK) mask = R.mask[i];
#pragma unroll
    for (int q = 0; q < kGCols; q++) {
      if (q < T.n) {
        const GCol c = T.c[q];
        if (c.groupbit == 0 || (mask & c.groupbit)) {
          double v = g_value(c, i, xr, vm, om, f, tq);
          if (c.op() == GO_SUMSQ) v = v * v;
          acc[q] = g_combine(c.op(), acc[q], v);
        }
      }
    }
  }
  // (c is a compile-time constant in the wave tree and threadIdx.x in the last step: the select keeps the table out of
  // runtime indexing, which would put it into scratch)
  auto comb = [&](int c, double a, double b) {
    int op = GO_SUM;
#pragma unroll
    for (int q = 0; q < kGCols; q++)
      if (q == c) op = T.c[q].op();
    return g_combine(op, a, b);
  };
  block_reduce_store<kGBlock, kGCols>(acc, partial + (size_t)kGCols * blockIdx.x, T.n, comb);
}

__global__ __launch_bounds__(kGBlock) void k_global_fold(const double* partial, int nb, GFold F, double rowcount)
{
  __shared__ double folded[kGCols], fin[kGCols];
  double v[kGCols];
#pragma unroll
  for (int q = 0; q < kGCols; q++) v[q] = q < F.n ? g_identity(F.op[q]) : 0.0;
  for (int b = threadIdx.x; b < nb; b += kGBlock)
#pragma unroll
    for (int q = 0; q < kGCols; q++)
      if (q < F.n) v[q] = g_combine(F.op[q], v[q], partial[(size_t)kGCols * b + q]);
  auto comb = [&](int c, double a, double b) {
    int op = GO_SUM;
#pragma unroll
    for (int q = 0; q < kGCols; q++)
      if (q == c) op = F.op[q];
    return g_combine(op, a, b);
  };
  block_reduce_store<kGBlock, kGCols>(v, folded, F.n, comb);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < F.n) {
    int div = -1;
    double* out = nullptr;
#pragma unroll
    for (int q = 0; q < kGCols; q++)
      if (q == t) {
        div = F.div[q];
        out = F.out[q];
      }
    double r = folded[t];
    const double cnt = div == -2 ? rowcount : (div >= 0 ? folded[div] : 0.0);
    if (cnt > 0.0) r = r / cnt;
    fin[t] = r;
    if (out) *out = r;
  }
  __syncthreads();
  if (t < F.nacc) {   // the samples of fix ave/time due at this step: one addition per (fix, value), in sample order
    int col = 0;
    double* dst = nullptr;
#pragma unroll
    for (int a = 0; a < kGAcc; a++)
      if (a == t) {
        col = F.acc_col[a];
        dst = F.acc_dst[a];
      }
    *dst += fin[col];
  }
}

// fix ave/time mode vector: column `src` (stride ncols) of a global array is added into column j of the accumulator
// [nrows][nv] -- one addition per element per sample
__global__ __launch_bounds__(kGBlock) void k_global_col_acc(const double* src, int ncols, int nrows, double* acc, int nv)
{
  const int r = blockIdx.x * kGBlock + threadIdx.x;
  if (r < nrows) acc[(size_t)r * nv] += src[(size_t)r * ncols];
}

__global__ __launch_bounds__(64) void k_global_acc(GAccOnly A)
{
  const int t = threadIdx.x;
  if (t >= A.n) return;
  const double* src = nullptr;
  double* dst = nullptr;
#pragma unroll
  for (int a = 0; a < kGAcc; a++)
    if (a == t) {
      src = A.src[a];
      dst = A.dst[a];
    }
  *dst += *src;
}

// ---- compute com ----

constexpr int kUCols = 4;   // sum m xu, m yu, m zu, m
struct UArgs {
  const double4* xr;
  const double4* vm;
  const int* mask;
  const int* tag;
  int groupbit;
  ImageView V;
};

// grid: the element count alone decides it (at least one block, which then stores the zeros of an empty bed); partial:
// [gridDim.x][kUCols]; ticket: zero before the launch and again after it; out: three values
__global__ __launch_bounds__(kGBlock) void k_global_unwrapped(UArgs A, long long n, double* partial, unsigned* ticket,
                                                              double* out)
{
  __shared__ int last;
  __shared__ double folded[kUCols];
  double acc[kUCols] = {0.0, 0.0, 0.0, 0.0};
  const long long stride = (long long)gridDim.x * kGBlock;
  for (long long i = (long long)blockIdx.x * kGBlock + threadIdx.x; i < n; i += stride) {
    if (!(A.mask[i] & A.groupbit)) continue;
    int im[3];
    double xu[3];
    image_of(A.V, A.tag[i], im);
    unmap(A.xr[i], im, A.V, xu);
    const double m = A.vm[i].w;
    acc[0] += xu[0] * m;
    acc[1] += xu[1] * m;
    acc[2] += xu[2] * m;
    acc[3] += m;
  }
  auto add = [](int, double a, double b) { return a + b; };
  block_reduce_store<kGBlock, kUCols>(acc, partial + (size_t)kUCols * blockIdx.x, kUCols, add);
  // this block's row is published before its ticket is drawn: every storing wave's stores have left, then one agent-scope
  // release (the per-XCD L2s are not coherent), then the relaxed add; the block that draws the last ticket acquires once
  // and reads every row with plain loads.  (The waits written out next to the fences repeat what the fences are meant to
  // emit: the compiler has been seen to drop a fence's own wait where it believes no store is in flight, and the ticket
  // must never overtake the row.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = drawn == gridDim.x - 1 ? 1 : 0;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  // the fold: thread t adds rows t, t + 256, ... in that order, then the same tree -- which block does it changes nothing.
  // (The second block_reduce_store of this kernel, the same instantiation and so the same LDS rows as the first: the two
  // barriers above lie between the first call's reads of those rows and this call's writes -- sf_block_reduce.h.)
  double v[kUCols] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < (int)gridDim.x; b += kGBlock)
#pragma unroll
    for (int q = 0; q < kUCols; q++) v[q] += partial[(size_t)kUCols * b + q];
  block_reduce_store<kGBlock, kUCols>(v, folded, kUCols, add);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double m = folded[3];
    for (int q = 0; q < 3; q++) out[q] = m > 0.0 ? folded[q] / m : 0.0;   // (a group of no atoms: zeros)
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- compute cluster/stats ----

// cnt[t]: the group atoms whose cluster ID (column 1 of a compute cluster/atom: a tag, or 0) is t; rows: the largest tag + 1
__global__ __launch_bounds__(kGBlock) void k_cluster_rows(const double* cid, const int* mask, int groupbit, int n, int rows,
                                                          int* cnt)
{
  const int i = blockIdx.x * kGBlock + threadIdx.x;
  if (i >= n || !(mask[i] & groupbit)) return;
  const int t = (int)cid[i];
  if (t > 0 && t < rows) atomicAdd(&cnt[t], 1);
}

constexpr int kSCols = 3;   // rows that are not zero, the largest row, the sum of the rows
// The hand-over of k_global_unwrapped: one partial row per block, an integer ticket behind an agent-scope release, the fold in
// the block that arrives last.  Every value is an integer below 2^31 carried in a double: exact in any order
__global__ __launch_bounds__(kGBlock) void k_cluster_stats(const int* cnt, int rows, double* partial, unsigned* ticket, double* out)
{
  __shared__ int last;
  __shared__ double folded[kSCols];
  double acc[kSCols] = {0.0, 0.0, 0.0};
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * kGBlock;
  // (the trip count is the same for every lane of a wave: the ballot sees the whole wave, and lane 0 adds its count)
  for (long long base = (long long)blockIdx.x * kGBlock + (threadIdx.x - lane); base < rows; base += stride) {
    const long long r = base + lane;
    const int c = r < rows ? cnt[r] : 0;
    const int nz = __popcll(__ballot(c > 0));
    if (lane == 0) acc[0] += (double)nz;
    acc[1] = fmax(acc[1], (double)c);
    acc[2] += (double)c;
  }
  auto comb = [](int q, double a, double b) { return q == 1 ? fmax(a, b) : a + b; };
  block_reduce_store<kGBlock, kSCols>(acc, partial + (size_t)kSCols * blockIdx.x, kSCols, comb);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = drawn == gridDim.x - 1 ? 1 : 0;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  double v[kSCols] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < (int)gridDim.x; b += kGBlock) {
    v[0] += partial[(size_t)kSCols * b];
    v[1] = fmax(v[1], partial[(size_t)kSCols * b + 1]);
    v[2] += partial[(size_t)kSCols * b + 2];
  }
  block_reduce_store<kGBlock, kSCols>(v, folded, kSCols, comb);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 0; q < kSCols; q++) out[q] = folded[q];
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- host side ----

enum GKind { G_REDUCE, G_KE, G_EROTATE, G_COM, G_CLUSTER };
constexpr int kNumGKinds = 5;
const char* const kStyleName[kNumGKinds] = {"reduce", "ke", "erotate/sphere", "com", "cluster/stats"};

struct GlobalCompute {
  std::string id;
  GKind kind = G_REDUCE;
  int groupbit = 1;
  ReduceSpec S;
  int nvalues = 1;
  int slot = -1;   // in the pool
  StateStamp made;   // what the values were made at
  std::string cid;           // G_CLUSTER: the compute cluster/atom it reads
  DeviceScratch tag_rows;    // G_CLUSTER: the integer counter per tag
  bool unwrapped() const { return kind == G_COM; }
  bool own_launches() const { return kind == G_COM || kind == G_CLUSTER; }   // not a column of k_global_gather
  bool is_vector() const { return own_launches() || (kind == G_REDUCE && S.inputs.size() > 1); }
  bool extensive() const { return !own_launches() && (kind != G_REDUCE || S.mode == GM_SUM || S.mode == GM_SUMSQ); }
};

struct AveTimeFix : AveFixState {
  AveTimeSpec S;
  int slot = -1;   // the accumulator, [nvalues] in the pool
  std::deque<std::vector<double>> blocks;   // ave window: the last M blocks
  std::vector<double> runsum;               // ave running: the sum of all blocks
  long long noutputs = 0;
  std::vector<double> values;   // the latest output (mode vector: row-major [nrows][nvalues])
  // mode vector: the columns of global arrays with nrows rows; the accumulator [nrows][nvalues] is an allocation of its own
  int nrows = 0;
  double* vacc = nullptr;
  std::vector<double> h_vacc;
  size_t nacc() const { return S.mode_vector ? (size_t)nrows * S.values.size() : S.values.size(); }
  ~AveTimeFix()
  {
    if (vacc) (void)hipFree(vacc);
  }
};

struct GlobalSet {
  std::vector<std::unique_ptr<GlobalCompute>> computes;
  std::vector<std::unique_ptr<AveTimeFix>> fixes;
  double* pool = nullptr;
  std::vector<char> used = std::vector<char>(kPool, 0);
  double* partial = nullptr;   // [kGMaxBlocks][kGCols]
  unsigned* ticket = nullptr;  // k_global_unwrapped: zero between launches
  double* h_buf = nullptr;     // pinned [kAveTimeMaxValues]
  long long launches = 0, host_copies = 0;
  ~GlobalSet()
  {
    if (pool) (void)hipFree(pool);
    if (partial) (void)hipFree(partial);
    if (ticket) (void)hipFree(ticket);
    if (h_buf) (void)hipHostFree(h_buf);
  }
  GlobalCompute* find(const std::string& id)
  {
    for (auto& c : computes)
      if (c->id == id) return c.get();
    return nullptr;
  }
  AveTimeFix* find_fix(const std::string& id) const { return ave_find(fixes, id); }
  void device(hipStream_t st)
  {
    if (pool) return;
    SF_HIP(hipMalloc(&pool, sizeof(double) * kPool));
    SF_HIP(hipMemsetAsync(pool, 0, sizeof(double) * kPool, st));
    SF_HIP(hipMalloc(&partial, sizeof(double) * kGMaxBlocks * kGCols));
    SF_HIP(hipMalloc(&ticket, sizeof(unsigned)));
    SF_HIP(hipMemsetAsync(ticket, 0, sizeof(unsigned), st));
    SF_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_buf), sizeof(double) * kAveTimeMaxValues));
  }
  int take(int n)   // n consecutive doubles of the pool, first fit
  {
    for (int s = 0; s + n <= kPool; s++) {
      int k = 0;
      while (k < n && !used[s + k]) k++;
      if (k == n) {
        std::fill(used.begin() + s, used.begin() + s + n, 1);
        return s;
      }
      s += k;
    }
    fail("too many global compute values and fix ave/time accumulators (%d doubles in all)", kPool);
  }
  void give(int s, int n)
  {
    if (s >= 0) std::fill(used.begin() + s, used.begin() + s + n, 0);
  }
};

GlobalSet* set_of(const SfLammps& L) { return L.globals.get<GlobalSet>(); }
GlobalSet& ensure_set(SfLammps& L) { return L.globals.ensure<GlobalSet>(); }

std::string who_of(const GlobalCompute& c) { return std::string("compute ") + kStyleName[c.kind]; }

// a c_ input of compute reduce: checked at the compute line and again at every evaluation (the compute may have been
// removed and defined anew).  Returns true for a compute pair/local, false for a per-atom compute
bool reduce_input_is_local(const SfLammps& L, const ReduceInput& in)
{
  const ComputeShape shape = compute_shape(L, in.id);
  fail_if(check_reduce_input(shape, in.index, in.id));
  return shape.kind == CK_LOCAL;
}

// ---- the plan ----

struct PlanCol {
  GCol col;
  bool ave = false;        // divided by the count of its group / of the rows
  int row_value = 0;       // a row column: which of the values typed on the pair/local line
  double* out = nullptr;
  std::vector<double*> acc;
};
struct AccReq {   // a sample of a fix: value `value` of compute c is added into *dst
  const GlobalCompute* c;
  int value;
  double* dst;
};

GOp op_of(int mode)
{
  switch (mode) {
    case GM_MIN: return GO_MIN;
    case GM_MAX: return GO_MAX;
    case GM_SUMSQ:
    case GM_AVESQ: return GO_SUMSQ;
    default: return GO_SUM;
  }
}

// gather + fold of up to kGCols columns (count columns included) over n elements
void launch_group(SfLammps& L, GlobalSet& G, const GTable& T, GFold& F, long long n, double rowcount)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int nb = n > 0 ? (int)std::min<long long>(kGMaxBlocks, (n + kGBlock - 1) / kGBlock) : 0;
  if (nb > 0) {
    GRecords R{e.d_xr(), e.d_vm(), e.d_om(), e.d_force(), e.d_torque(), e.d_mask()};
    k_global_gather<<<nb, kGBlock, 0, st>>>(R, T, n, G.partial);
    G.launches++;
  }
  k_global_fold<<<1, kGBlock, 0, st>>>(G.partial, nb, F, rowcount);
  SF_HIP(hipGetLastError());
  G.launches++;
}

// the columns `cols` over n elements, in launches of at most kGCols columns; rows: ave divides by the row count
void launch_columns(SfLammps& L, GlobalSet& G, const std::vector<PlanCol>& cols, long long n, bool rows,
                    std::vector<std::pair<const double*, double*>>* late_acc)
{
  size_t k = 0;
  while (k < cols.size()) {
    GTable T{};
    GFold F{};
    int count_of[kGCols];   // the group bit a count column counts (0: not a count column)
    for (int q = 0; q < kGCols; q++) count_of[q] = 0, F.div[q] = -1, F.out[q] = nullptr;
    while (k < cols.size()) {
      const PlanCol& pc = cols[k];
      int cq = -1;
      if (pc.ave && !rows)
        for (int q = 0; q < T.n; q++)
          if (count_of[q] == pc.col.groupbit) cq = q;
      const int more = 1 + (pc.ave && !rows && cq < 0 ? 1 : 0);
      if (T.n + more > kGCols) break;
      if (pc.ave && !rows && cq < 0) {
        cq = T.n++;
        T.c[cq] = make_col(nullptr, GS_ONE, 0, pc.col.groupbit, GO_SUM);
        count_of[cq] = pc.col.groupbit;
      }
      const int q = T.n++;
      T.c[q] = pc.col;
      F.div[q] = pc.ave ? (rows ? -2 : cq) : -1;
      F.out[q] = pc.out;
      for (double* dst : pc.acc) {
        if (F.nacc < kGAcc) {
          F.acc_col[F.nacc] = q;
          F.acc_dst[F.nacc] = dst;
          F.nacc++;
        } else
          late_acc->push_back({pc.out, dst});
      }
      k++;
    }
    F.n = T.n;
    for (int q = 0; q < T.n; q++) {
      F.op[q] = T.c[q].op();
      T.need |= need_of(T.c[q]);
    }
    launch_group(L, G, T, F, n, (double)n);
  }
}

void launch_late_acc(SfLammps& L, GlobalSet& G, const std::vector<std::pair<const double*, double*>>& late)
{
  for (size_t k = 0; k < late.size(); k += kGAcc) {
    GAccOnly A{};
    A.n = (int)std::min<size_t>(kGAcc, late.size() - k);
    for (int a = 0; a < A.n; a++) {
      A.src[a] = late[k + a].first;
      A.dst[a] = late[k + a].second;
    }
    k_global_acc<<<1, 64, 0, L.eng.stream()>>>(A);
    SF_HIP(hipGetLastError());
    G.launches++;
  }
}

// compute com: one launch of k_global_unwrapped over the owned atoms
void evaluate_unwrapped(SfLammps& L, GlobalSet& G, GlobalCompute& c)
{
  const ImageView V = image_view(L, who_of(c).c_str());
  DemEngine& e = L.eng;
  const long long n = e.nlocal();
  const int nb = (int)std::max<long long>(1, std::min<long long>(kGMaxBlocks, (n + kGBlock - 1) / kGBlock));
  const UArgs A{e.d_xr(), e.d_vm(), e.d_mask(), e.d_tag(), c.groupbit, V};
  k_global_unwrapped<<<nb, kGBlock, 0, e.stream()>>>(A, n, G.partial, G.ticket, G.pool + c.slot);
  SF_HIP(hipGetLastError());
  G.launches++;
}

// CID of a compute cluster/stats: checked at the compute line and again at every evaluation (the compute may have been removed
// or defined anew as something else)
void check_cluster_id(const SfLammps& L, const std::string& cid)
{
  if (compute_shape(L, cid).kind == CK_NONE) fail("compute cluster/stats: Could not find compute ID %s", cid.c_str());
  if (!atom_compute_cluster_spec(L, cid, nullptr, nullptr))
    fail("compute cluster/stats: compute %s is not a compute cluster/atom", cid.c_str());
}

// compute cluster/stats: the counter per tag is zeroed, takes the atoms, and is reduced by one launch
void evaluate_cluster_stats(SfLammps& L, GlobalSet& G, GlobalCompute& c)
{
  check_cluster_id(L, c.cid);
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int n = e.nlocal();
  int nc = 0;
  const double* cid = atom_compute_values(L, c.cid, &nc);   // (once per step however many ask; column 1 comes first)
  const int rows = e.max_tag() + 1;
  int* cnt = static_cast<int*>(c.tag_rows.get(sizeof(int) * (size_t)rows, st));
  SF_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)rows, st));
  if (n > 0) {
    k_cluster_rows<<<div_up(n, kGBlock), kGBlock, 0, st>>>(cid, e.d_mask(), c.groupbit, n, rows, cnt);
    G.launches++;
  }
  const int nb = std::max(1, std::min(kGMaxBlocks, div_up(rows, kGBlock)));
  k_cluster_stats<<<nb, kGBlock, 0, st>>>(cnt, rows, G.partial, G.ticket, G.pool + c.slot);
  SF_HIP(hipGetLastError());
  G.launches++;
}

// Every compute of `want` that is stale is evaluated, once; `accs`: the additions of the fix samples due now, carried by
// the fold launches of the values they name (or by k_global_acc where the value was evaluated at this step before)
void evaluate(SfLammps& L, GlobalSet& G, const std::vector<GlobalCompute*>& want, const std::vector<AccReq>& accs)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  G.device(st);
  const int n = e.nlocal();
  std::vector<PlanCol> atom_cols;
  std::vector<std::pair<std::string, std::vector<PlanCol>>> row_cols;   // per compute pair/local
  std::vector<std::pair<const double*, double*>> late;
  std::vector<GlobalCompute*> stale;
  for (GlobalCompute* c : want) {
    refuse_decomposed(L, who_of(*c).c_str());
    if (std::find(stale.begin(), stale.end(), c) != stale.end()) continue;
    if (c->made.is_now(e)) continue;
    stale.push_back(c);
  }
  for (const AccReq& a : accs)
    if (std::find(stale.begin(), stale.end(), a.c) == stale.end()) late.push_back({G.pool + a.c->slot + a.value, a.dst});
  for (GlobalCompute* c : stale) {
    if (c->own_launches()) {   // (the samples of the fixes are added behind them)
      if (c->unwrapped()) evaluate_unwrapped(L, G, *c);
      else evaluate_cluster_stats(L, G, *c);
      for (const AccReq& a : accs)
        if (a.c == c) late.push_back({G.pool + c->slot + a.value, a.dst});
      continue;
    }
    for (int j = 0; j < c->nvalues; j++) {
      PlanCol pc;
      pc.out = G.pool + c->slot + j;
      for (const AccReq& a : accs)
        if (a.c == c && a.value == j) pc.acc.push_back(a.dst);
      pc.col = make_col(nullptr, GS_ZERO, 0, c->groupbit, GO_SUM);
      if (c->kind == G_KE) pc.col.set(GS_KE, 0, GO_SUM);
      else if (c->kind == G_EROTATE) pc.col.set(GS_EROT, 0, GO_SUM);
      else {
        const ReduceInput& in = c->S.inputs[j];
        const GOp op = op_of(c->S.mode);
        pc.ave = c->S.mode == GM_AVE || c->S.mode == GM_AVESQ;
        if (in.attr != AA_COMPUTE) {
          pc.col.set(in.attr < AA_VX ? GS_XR : (in.attr < AA_FX ? GS_VM : GS_FORCE), in.attr % 3, op);
        } else if (!reduce_input_is_local(L, in)) {
          int nc = 0;
          const double* val = atom_compute_values(L, in.id, &nc);   // (once per step however many ask)
          pc.col.set(GS_PTR, 0, op);
          pc.col.p = val ? val + (size_t)(in.index > 0 ? in.index - 1 : 0) * (size_t)n : nullptr;
        } else {
          pc.col.groupbit = 0;   // every row, whatever the group of the reduce
          pc.col.set(GS_ZERO, 0, op);
          pc.row_value = (int)(in.index > 0 ? in.index - 1 : 0);   // (the source is filled in once the rows exist)
          size_t r = 0;
          while (r < row_cols.size() && row_cols[r].first != in.id) r++;
          if (r == row_cols.size()) row_cols.push_back({in.id, {}});
          row_cols[r].second.push_back(pc);
          continue;
        }
      }
      atom_cols.push_back(pc);
    }
  }
  launch_columns(L, G, atom_cols, n, false, &late);
  for (auto& rc : row_cols) {
    std::vector<unsigned char> values;
    int groupbit = 1;
    compute_lookup(L, rc.first, &values, &groupbit);
    const ContactRows R = contact_rows(L, groupbit);   // (reads the row count on the host: one wait)
    for (PlanCol& pc : rc.second) {
      const int v = values[pc.row_value];
      const int op = pc.col.op();
      if (v < kContactDoubles) {
        pc.col.set(GS_PTR, 0, op);
        pc.col.p = R.val ? R.val + (size_t)v * (size_t)R.n : nullptr;
      } else if (v == CV_TAG1 || v == CV_TAG2) {
        pc.col.set(GS_INT, 0, op);
        pc.col.p = v == CV_TAG1 ? R.tag1 : R.tag2;
      } else
        pc.col.set(GS_ZERO, 0, op);   // eng
    }
    launch_columns(L, G, rc.second, R.n, true, &late);   // (before the next compute's rows take the same buffers)
  }
  launch_late_acc(L, G, late);
  for (GlobalCompute* c : stale) c->made.set(e);
}

void copy_to_host(SfLammps& L, GlobalSet& G, int slot, int n, bool zero_after)
{
  hipStream_t st = L.eng.stream();
  SF_HIP(hipMemcpyAsync(G.h_buf, G.pool + slot, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  if (zero_after) SF_HIP(hipMemsetAsync(G.pool + slot, 0, sizeof(double) * (size_t)n, st));
  SF_HIP(hipStreamSynchronize(st));
  G.host_copies++;
}

// ---- fix ave/time ----

// checked at the fix line and again at every sample (the compute may have been redefined)
void check_fix_value(const SfLammps& L, const AveTimeValue& v)
{
  fail_if(check_ave_time_scalar(compute_shape(L, v.id), v.index));
}

// mode vector: c_ID[k] is column k of a global array; every value of a fix has the same number of rows, which is returned.
// Checked at the fix line and again at every sample
int check_fix_column(SfLammps& L, const AveTimeValue& v, int nrows, int* ncols = nullptr)
{
  pchunk_prepare(L, v.id);   // (a per-chunk compute knows its rows once its chunk/atom compute is evaluated)
  const ComputeShape shape = compute_shape(L, v.id);
  fail_if(check_ave_time_vector(shape, v.index, nrows));
  if (ncols) *ncols = shape.n;
  return shape.rows;
}

void write_line(AveTimeFix& F)
{
  FILE* fp = F.file.fp();
  if (!fp) return;
  fail_if(F.file.begin_block());
  if (F.S.mode_vector) {   // `step nrows`, then one line per row: the row number from 1 and its values
    const size_t nv = F.S.values.size();
    fprintf(fp, "%lld %d\n", F.out_step, F.nrows);
    for (int r = 0; r < F.nrows; r++) {
      fprintf(fp, "%d", r + 1);
      for (size_t j = 0; j < nv; j++) fprintf(fp, F.S.format.c_str(), F.values[(size_t)r * nv + j]);
      fputc('\n', fp);
    }
  } else {
    fprintf(fp, "%lld", F.out_step);
    for (double v : F.values) fprintf(fp, F.S.format.c_str(), v);
    fputc('\n', fp);
  }
  fail_if(F.file.end_block());
}

// the accumulator of Nrepeat samples -> one output (divided on the host)
void make_output(SfLammps& L, GlobalSet& G, AveTimeFix& F)
{
  const int nv = (int)F.nacc();
  const double* h = G.h_buf;
  if (F.S.mode_vector) {   // (its accumulator is larger than the pinned buffer of the scalar values)
    hipStream_t st = L.eng.stream();
    F.h_vacc.resize((size_t)nv);
    SF_HIP(hipMemcpyAsync(F.h_vacc.data(), F.vacc, sizeof(double) * (size_t)nv, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemsetAsync(F.vacc, 0, sizeof(double) * (size_t)nv, st));
    SF_HIP(hipStreamSynchronize(st));
    G.host_copies++;
    h = F.h_vacc.data();
  } else
    copy_to_host(L, G, F.slot, nv, true);
  std::vector<double> block(nv);
  const double nrep = (double)F.S.nrepeat;
  for (int j = 0; j < nv; j++) block[j] = h[j] / nrep;
  F.noutputs++;
  F.values.assign(nv, 0.0);
  if (F.S.ave == AVE_ONE) F.values = block;
  else if (F.S.ave == AVE_RUNNING) {
    if (F.runsum.empty()) F.runsum.assign(nv, 0.0);
    for (int j = 0; j < nv; j++) {
      F.runsum[j] += block[j];
      F.values[j] = F.runsum[j] / (double)F.noutputs;
    }
  } else {
    F.blocks.push_back(block);
    if ((long)F.blocks.size() > F.S.window) F.blocks.pop_front();
    for (int j = 0; j < nv; j++) {
      double s = 0.0;
      for (const auto& b : F.blocks) s += b[j];   // (oldest first)
      F.values[j] = s / (double)F.blocks.size();
    }
  }
  F.out_step = L.eng.nsteps();
  F.have = true;
  write_line(F);
}

bool fix_exists(const SfLammps& L, const std::string& id)
{
  GlobalSet* G = set_of(L);
  return G && G->find_fix(id);
}

bool unfix(SfLammps& L, const std::string& id)
{
  GlobalSet* G = set_of(L);
  const std::unique_ptr<AveTimeFix> f = G ? ave_take(L, G->fixes, id) : nullptr;
  if (f && !f->S.mode_vector) G->give(f->slot, (int)f->S.values.size());
  return f != nullptr;
}

bool fix_uses_compute(const SfLammps& L, const std::string& id)
{
  const GlobalSet* G = set_of(L);
  if (!G) return false;
  for (const auto& f : G->fixes)
    for (const AveTimeValue& v : f->S.values)
      if (v.id == id) return true;
  return false;
}

long long next_step(const SfLammps& L, long long step)
{
  const GlobalSet* G = set_of(L);
  return G ? ave_next(G->fixes, step) : -1;
}

GlobalCompute& compute_of(GlobalSet& G, const std::string& id, const char* missing)
{
  GlobalCompute* c = G.find(id);
  if (!c) fail("%s", missing);
  return *c;
}

// ---- the computes: the kind (sf_compute_ids.h) ----

bool is_style(const std::string& style)
{
  if (style == "reduce/region") return true;   // (refused by name in define)
  for (const char* s : kStyleName)
    if (style == s) return true;
  return false;
}

void define(SfLammps& L, const std::vector<std::string>& w)
{
  if (w[3] == "reduce/region") fail("compute reduce/region is not supported: compute reduce on a region group is (group ID region RID, or group ID dynamic)");
  auto c = std::make_unique<GlobalCompute>();
  c->id = w[1];
  c->groupbit = L.eng.group_bit(w[2]);
  for (int k = 0; k < kNumGKinds; k++)
    if (w[3] == kStyleName[k]) c->kind = (GKind)k;
  refuse_decomposed(L, who_of(*c).c_str());
  if (c->kind == G_REDUCE) {
    fail_if(parse_reduce(w, &c->S));
    for (const ReduceInput& in : c->S.inputs)
      if (in.attr == AA_COMPUTE) reduce_input_is_local(L, in);
    c->nvalues = (int)c->S.inputs.size();
  } else if (c->kind == G_COM) {
    fail_if(parse_com(w));
    c->nvalues = 3;
  } else if (c->kind == G_CLUSTER) {
    fail_if(parse_cluster_stats(w, &c->cid));
    check_cluster_id(L, c->cid);
    c->nvalues = 3;
  } else if (w.size() != 4)
    fail("Illegal compute %s command", w[3].c_str());
  GlobalSet& G = ensure_set(L);
  if (c->unwrapped()) (void)image_view(L, who_of(*c).c_str());   // (refused where image counts cannot be kept; makes the table)
  c->slot = G.take(c->nvalues);
  G.computes.push_back(std::move(c));
}

bool shape(const SfLammps& L, const std::string& id, ComputeShape* s)
{
  GlobalSet* G = set_of(L);
  const GlobalCompute* c = G ? G->find(id) : nullptr;
  if (!c) return false;
  *s = ComputeShape();
  s->kind = CK_GLOBAL;
  s->n = c->nvalues;
  s->vector = c->is_vector();
  return true;
}

void remove(SfLammps& L, const std::string& id)
{
  GlobalSet* G = set_of(L);
  // (a launch queued on the stream may still write its values)
  if (const std::unique_ptr<GlobalCompute> c = G ? compute_take(L, G->computes, id) : nullptr) G->give(c->slot, c->nvalues);
}

void invalidate(SfLammps& L)
{
  if (GlobalSet* G = set_of(L))
    for (auto& c : G->computes) c->made.clear();
}

}  // namespace

const AveFixKind& ave_time_kind()
{
  static const AveFixKind kind = {"fix ave/time", fix_exists, unfix, fix_uses_compute, next_step};
  return kind;
}

const ComputeKindOps& global_compute_kind()
{
  static const ComputeKindOps kind = {is_style, define, remove, shape, invalidate};
  return kind;
}

bool global_compute_extensive(const SfLammps& L, const std::string& id)
{
  GlobalSet* G = set_of(L);
  const GlobalCompute* c = G ? G->find(id) : nullptr;
  return c && c->extensive();
}

bool reduce_uses_compute(const SfLammps& L, const std::string& id)
{
  const GlobalSet* G = set_of(L);
  if (!G) return false;
  for (const auto& c : G->computes)
    if (c->kind == G_REDUCE)
      for (const ReduceInput& in : c->S.inputs)
        if (in.attr == AA_COMPUTE && in.id == id) return true;
  return false;
}

void global_values_host(SfLammps& L, const std::string& id, std::vector<double>* out)
{
  GlobalSet* G = set_of(L);
  GlobalCompute* c = G ? G->find(id) : nullptr;
  if (!c) fail("Could not find compute ID %s", id.c_str());
  evaluate(L, *G, {c}, {});
  copy_to_host(L, *G, c->slot, c->nvalues, false);
  out->assign(G->h_buf, G->h_buf + c->nvalues);
}

const double* global_values_device(SfLammps& L, const std::string& id)
{
  GlobalSet* G = set_of(L);
  GlobalCompute* c = G ? G->find(id) : nullptr;
  if (!c) fail("Could not find compute ID %s", id.c_str());
  evaluate(L, *G, {c}, {});
  return G->pool + c->slot;
}

// ---- the fix ----

void ave_time_fix_command(SfLammps& L, const std::string& line)
{
  std::vector<std::string> w;
  const std::string qerr = split_quoted(line, &w);
  if (!qerr.empty()) fail("%s", qerr.c_str());
  auto F = std::make_unique<AveTimeFix>();
  fail_if(parse_ave_time(w, &F->S));
  refuse_decomposed(L, "fix ave/time");
  (void)L.eng.group_bit(F->S.group);   // (the group must exist; it is not used, as in LAMMPS)
  GlobalSet& G = ensure_set(L);
  if (ave_fix_exists(L, F->S.id))
    fail("fix ave/time %s: this fix ID is in use (unfix it first)", F->S.id.c_str());
  if (F->S.mode_vector)
    for (const AveTimeValue& v : F->S.values) F->nrows = check_fix_column(L, v, F->nrows);
  else
    for (const AveTimeValue& v : F->S.values) check_fix_value(L, v);
  hipStream_t st = L.eng.stream();
  G.device(st);
  const int nv = (int)F->S.values.size();
  F->S.begin(L.eng.nsteps());
  std::string titles[3] = {"# Time-averaged data for fix " + F->S.id, "# TimeStep", ave_time_title3(F->S)};
  if (F->S.mode_vector) titles[1] += " Number-of-rows";
  else
    for (const AveTimeValue& v : F->S.values) titles[1] += " " + v.word;
  fail_if(F->file.open(F->S, "ave/time", F->S.id, titles, F->S.mode_vector ? 3 : 2));
  if (F->S.mode_vector) {
    SF_HIP(hipMalloc(&F->vacc, sizeof(double) * F->nacc()));
    SF_HIP(hipMemsetAsync(F->vacc, 0, sizeof(double) * F->nacc(), st));
  } else {
    F->slot = G.take(nv);
    SF_HIP(hipMemsetAsync(G.pool + F->slot, 0, sizeof(double) * (size_t)nv, st));
  }
  G.fixes.push_back(std::move(F));
}

void global_step_due(SfLammps& L, const std::vector<std::string>& also)
{
  GlobalSet* G = set_of(L);
  if (!G) return;
  const long long step = L.eng.nsteps();
  std::vector<AveTimeFix*> due;
  for (auto& f : G->fixes) {
    if (f->S.catch_up(step))   // (the samples of the output that was under way are dropped)
      SF_HIP(hipMemsetAsync(f->S.mode_vector ? f->vacc : G->pool + f->slot, 0, sizeof(double) * f->nacc(), L.eng.stream()));
    if (f->S.due(step)) due.push_back(f.get());
  }
  if (due.empty() && also.empty()) return;
  if (!due.empty()) refuse_decomposed(L, "fix ave/time");
  std::vector<GlobalCompute*> want;
  std::vector<AccReq> accs;
  for (AveTimeFix* f : due) {
    if (f->S.mode_vector) {   // the columns of global arrays: each array evaluated once per step (sf_nbr.hip), no host copy
      const int nv = (int)f->S.values.size();
      for (int j = 0; j < nv; j++) {
        const AveTimeValue& v = f->S.values[j];
        int ncols = 0;
        check_fix_column(L, v, f->nrows, &ncols);
        const double* src = pchunk_holds(L, v.id) ? pchunk_array_device(L, v.id, nullptr, nullptr) : rdf_array_device(L, v.id);
        k_global_col_acc<<<div_up(f->nrows, kGBlock), kGBlock, 0, L.eng.stream()>>>(src + (v.index - 1), ncols, f->nrows,
                                                                                    f->vacc + j, nv);
        SF_HIP(hipGetLastError());
        G->launches++;
      }
      continue;
    }
    for (size_t j = 0; j < f->S.values.size(); j++) {
      const AveTimeValue& v = f->S.values[j];
      check_fix_value(L, v);
      GlobalCompute& c = compute_of(*G, v.id, "Compute ID for fix ave/time does not exist");
      want.push_back(&c);
      accs.push_back({&c, (int)(v.index > 0 ? v.index - 1 : 0), G->pool ? G->pool + f->slot + j : nullptr});
    }
  }
  for (const std::string& id : also) want.push_back(&compute_of(*G, id, "Could not find thermo custom compute ID"));
  evaluate(L, *G, want, accs);
  for (AveTimeFix* f : due)
    if (f->S.sampled(step)) make_output(L, *G, *f);
}

}  // namespace sf

using sf::handle;

extern "C" {

long long sf_lammps_compute_global(void* ptr, const char* id, long long max, double* values, int* is_vector)
{
  long long n = 0;
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id) sf::fail("sf_lammps_compute_global: null argument");
  const sf::ComputeShape shape = sf::compute_shape(L, id);
  sf::fail_if(sf::check_get_global(shape, id));
  n = shape.n;
  if (is_vector) *is_vector = shape.vector ? 1 : 0;
  if (n <= max) {
    if (!values) sf::fail("sf_lammps_compute_global: null argument");
    std::vector<double> v;
    sf::global_values_host(L, id, &v);
    std::copy(v.begin(), v.end(), values);
  }
  SF_API_END(n)
}

long long sf_lammps_ave_time(void* ptr, const char* id, long long max, long long* step, double* values)
{
  long long n = 0;
  SF_API_BEGIN
  if (!id) sf::fail("sf_lammps_ave_time: null argument");
  sf::GlobalSet* G = sf::set_of(*handle(ptr));
  sf::AveTimeFix* F = G ? G->find_fix(id) : nullptr;
  if (!F) sf::fail("Could not find fix ave/time ID %s", id);
  if (!F->have) sf::fail("fix ave/time %s has made no output yet (the first one is due at a multiple of Nfreq)", id);
  if (step) *step = F->out_step;
  n = (long long)F->values.size();
  if (n <= max) {
    if (!values) sf::fail("sf_lammps_ave_time: null argument");
    std::copy(F->values.begin(), F->values.end(), values);
  }
  SF_API_END(n)
}

// rows of a mode vector fix (sf_lammps_ave_time then returns [rows][nvalues] row-major); 0: a mode scalar fix
long long sf_lammps_ave_time_rows(void* ptr, const char* id)
{
  long long n = 0;
  SF_API_BEGIN
  if (!id) sf::fail("sf_lammps_ave_time_rows: null argument");
  sf::GlobalSet* G = sf::set_of(*handle(ptr));
  sf::AveTimeFix* F = G ? G->find_fix(id) : nullptr;
  if (!F) sf::fail("Could not find fix ave/time ID %s", id);
  n = F->S.mode_vector ? F->nrows : 0;
  SF_API_END(n)
}

long long sf_lammps_ave_time_names(void* ptr, const char* id, long long max, char* names)
{
  long long n = 0;
  SF_API_BEGIN
  if (!id) sf::fail("sf_lammps_ave_time_names: null argument");
  sf::GlobalSet* G = sf::set_of(*handle(ptr));
  sf::AveTimeFix* F = G ? G->find_fix(id) : nullptr;
  if (!F) sf::fail("Could not find fix ave/time ID %s", id);
  std::string s;
  for (const sf::AveTimeValue& v : F->S.values) s += (s.empty() ? "" : " ") + v.word;
  n = (long long)s.size() + 1;
  if (n <= max) {
    if (!names) sf::fail("sf_lammps_ave_time_names: null argument");
    std::memcpy(names, s.c_str(), (size_t)n);
  }
  SF_API_END(n)
}

int sf_lammps_global_launches(void* ptr, long long* launches, long long* host_copies)
{
  SF_API_BEGIN
  if (!launches) sf::fail("sf_lammps_global_launches: null argument");
  const sf::GlobalSet* G = sf::set_of(*handle(ptr));
  *launches = G ? G->launches : 0;
  if (host_copies) *host_copies = G ? G->host_copies : 0;
  SF_API_END(0)
}

int sf_lammps_global_cost(void* ptr, const char* id, double* ms)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id || !ms) sf::fail("sf_lammps_global_cost: null argument");
  sf::GlobalSet* G = sf::set_of(L);
  sf::GlobalCompute* c = G ? G->find(id) : nullptr;
  if (!c) sf::fail("Could not find compute ID %s", id);
  // (the per-atom computes behind c_ inputs are evaluated outside the time: sf_lammps_compute_atom_cost times them)
  sf::evaluate(L, *G, {c}, {});
  c->made.clear();
  *ms = sf::stream_ms(L.eng.stream(), [&] { sf::evaluate(L, *G, {c}, {}); });
  SF_API_END(0)
}

}  // extern "C"
