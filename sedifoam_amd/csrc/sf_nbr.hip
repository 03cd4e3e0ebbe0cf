// sf_nbr.hip -- a neighbourhood walk at the moment of an output: the atoms within a cutoff the user
// chooses of every owned atom, on the positions as they stand, behind
//   compute ID group rdf Nbin [itype jtype ...] cutoff Rc      g(r) and the running coordination number, a global array
//   compute ID group coord/atom cutoff Rc [typerange ...]      the atoms within Rc, by type (sf_compute_atom.hip registers it)
// ([3P] LAMMPS names and rules: ComputeRDF, ComputeCoordAtom).  The pair list of the run ends at the contact distance plus the
// skin and belongs to the last rebuild; this file has a grid of its own and touches neither the list, the rebuild nor the
// sub-step kernel.
//
// The grid, on the engine's stream:
//   k_nbr_keys    one lane per owned atom: its cell (edge >= Rc (1 + 2^-20) in every dimension; a periodic dimension wraps the
//                 index, so that an atom half a skin outside the box lands in the cell of its image; a non-periodic one
//                 clamps it), and an integer count of the cell
//   exclusive_scan_i32, sort_pairs_u32 (sf_sort.hip)          cell starts; the atoms in cell order, by index within a cell
//   k_nbr_pack    the compact copy in cell order: x y z and (type, group word) in one 32-byte record
// The walk, one lane per atom in cell order: its own cell and the adjacent ones (one cell: that cell; two: both, once), every
// record of a cell read by all lanes of that cell at once (one line, broadcast).  d = xj - xi, the minimum image applied
// once, rsq = (dx dx + dy dy) + dz dz with no contraction, sqrt rounded correctly.
//   k_nbr_rdf     ordered pairs of group atoms into per-block 32-bit LDS counters with LDS integer atomics (the wave whose
//                 counted lanes all share one bin adds once: sf_histo.hip), then into 64-bit device counters; the group atoms
//                 of each pair's type ranges are counted by ballots into the same counters
//   k_rdf_norm    one lane per pair: g(r) and ncoord, operation by operation in the order of the rule
//   k_nbr_coord   counts in registers, stored per atom
// Every tally is an integer, so the bits do not depend on the order of the additions; no floating-point atomics.
//
// On the same grid, `compute ID group cluster/atom CUT [surface no|yes] [size no|yes]` ([3P] ComputeClusterAtom; DESIGN.md
// section 21; sf_compute_atom.hip registers it): the connected components of "linked" as a union-find over the places of the
// cell order, one lane per place.
//   k_cl_init, k_cl_pack_radius   parent[p] = p for the group, -1 for the others; the radii in cell order (surface yes only)
//   k_cl_edges<false>             the hook launch: every linked pair, from its higher place, unites its two trees
//   k_cl_compress                 parent[p] = the root above p as the launch before left it
//   k_cl_edges<true>              the verify launch: the same walk, writing nothing unless a pair is still apart; then it
//                                 hooks it and raises a flag, and the host repeats compress + verify (at most 64 rounds)
//   k_cl_tally, k_cl_store        integer atomics per root (smallest tag, count), then the per-atom values
// What is and is not assumed about memory inside a launch stands above the kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_compute_atom.h"
#include "sf_compute_ids.h"
#include "sf_nbr.h"
#include "sf_pchunk.h"
#include "sf_unmap.h"

// (a*a + s stays a product and a sum: rsq has the same bits from both sides of a pair and in the NumPy statement)
#pragma clang fp contract(off)

namespace sf {
namespace {

constexpr int kNBlock = 256;

struct NbrGridDev {
  double lo[3], inv[3];    // cell = floor((x - lo) * inv)
  double prd[3], half[3];  // box lengths and 0.5 * them
  int nc[3];
  int periodic[3];
  int off0[3], noff[3];    // the cell offsets a walk visits in each dimension: off0 .. off0 + noff - 1
};

__device__ __forceinline__ int nbr_cell1(const NbrGridDev& G, int a, double x)
{
  double t = floor((x - G.lo[a]) * G.inv[a]);
  t = fmin(fmax(t, -1.0e9), 1.0e9);   // (a NaN or a far-away coordinate must not overflow the conversion)
  int c = (int)t;
  const int n = G.nc[a];
  if (G.periodic[a]) {
    c %= n;
    if (c < 0) c += n;
  } else
    c = min(max(c, 0), n - 1);
  return c;
}

__device__ __forceinline__ int nbr_cell(const NbrGridDev& G, double x, double y, double z, int* cx, int* cy, int* cz)
{
  *cx = nbr_cell1(G, 0, x);
  *cy = nbr_cell1(G, 1, y);
  *cz = nbr_cell1(G, 2, z);
  return (*cz * G.nc[1] + *cy) * G.nc[0] + *cx;
}

__global__ __launch_bounds__(kNBlock) void k_nbr_keys(NbrGridDev G, const double4* xr, int n, unsigned* key, int* idx, int* count)
{
  const int i = blockIdx.x * kNBlock + threadIdx.x;
  if (i >= n) return;
  const double4 x = xr[i];
  int cx, cy, cz;
  const int c = nbr_cell(G, x.x, x.y, x.z, &cx, &cy, &cz);
  key[i] = (unsigned)c;
  idx[i] = i;
  atomicAdd(&count[c], 1);
}

// pos[p]: x y z of the atom at place p of the cell order, and its type (low word) and group word (high word) in w
__global__ __launch_bounds__(kNBlock) void k_nbr_pack(const double4* xr, const int* type, const int* mask, const int* idx, int n,
                                                      double4* pos)
{
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  if (p >= n) return;
  const int i = idx[p];
  const double4 x = xr[i];
  const long long tw = (long long)(unsigned)type[i] | ((long long)(unsigned)mask[i] << 32);
  pos[p] = make_double4(x.x, x.y, x.z, __longlong_as_double(tw));
}

__device__ __forceinline__ int nbr_type(const double4& r) { return (int)(unsigned)(__double_as_longlong(r.w) & 0xffffffffll); }
__device__ __forceinline__ int nbr_mask(const double4& r) { return (int)(unsigned)((unsigned long long)__double_as_longlong(r.w) >> 32); }

// xj - xi with the minimum image applied once
__device__ __forceinline__ double nbr_delta(const NbrGridDev& G, int a, double xj, double xi)
{
  double d = xj - xi;
  if (G.periodic[a]) {
    if (d > G.half[a]) d -= G.prd[a];
    else if (d < -G.half[a]) d += G.prd[a];
  }
  return d;
}

// f(j, record of j, rsq) for every place j != p of the cell (cx, cy, cz) and of the adjacent cells, each cell once
template <class F>
__device__ __forceinline__ void nbr_walk_places(const NbrGridDev& G, const double4* pos, const int* start, int p,
                                                const double4& me, int cx, int cy, int cz, F&& f)
{
  for (int oz = 0; oz < G.noff[2]; oz++) {
    int z = cz + G.off0[2] + oz;
    if (G.periodic[2]) z = z < 0 ? z + G.nc[2] : (z >= G.nc[2] ? z - G.nc[2] : z);
    else if (z < 0 || z >= G.nc[2]) continue;
    for (int oy = 0; oy < G.noff[1]; oy++) {
      int y = cy + G.off0[1] + oy;
      if (G.periodic[1]) y = y < 0 ? y + G.nc[1] : (y >= G.nc[1] ? y - G.nc[1] : y);
      else if (y < 0 || y >= G.nc[1]) continue;
      for (int ox = 0; ox < G.noff[0]; ox++) {
        int x = cx + G.off0[0] + ox;
        if (G.periodic[0]) x = x < 0 ? x + G.nc[0] : (x >= G.nc[0] ? x - G.nc[0] : x);
        else if (x < 0 || x >= G.nc[0]) continue;
        const int c = (z * G.nc[1] + y) * G.nc[0] + x;
        const int end = start[c + 1];
        for (int j = start[c]; j < end; j++) {
          if (j == p) continue;
          const double4 o = pos[j];
          const double dx = nbr_delta(G, 0, o.x, me.x), dy = nbr_delta(G, 1, o.y, me.y), dz = nbr_delta(G, 2, o.z, me.z);
          const double rsq = (dx * dx + dy * dy) + dz * dz;
          f(j, o, rsq);
        }
      }
    }
  }
}

// ... for the walks that do not ask which place it is: f(record of j, rsq)
template <class F>
__device__ __forceinline__ void nbr_walk(const NbrGridDev& G, const double4* pos, const int* start, int p, const double4& me,
                                         int cx, int cy, int cz, F&& f)
{
  nbr_walk_places(G, pos, start, p, me, cx, cy, cz, [&](int, const double4& o, double rsq) { f(o, rsq); });
}

struct RdfArgs {
  int nbin, npairs, groupbit;
  double delrinv;
  double rsq_skip;     // above it a pair is beyond the last bin whatever the rounding: Rc^2 (1 + 1e-9)
  const int4* pairs;   // ilo ihi jlo jhi of each pair
};

// acc: [npairs][nbin] counts, then icount jcount duplicates of each pair.  Dynamic LDS: npairs * nbin counters of 32 bits --
// a block counts at most 256 n ordered pairs per counter, below 2^32 for every n below 2^24
__global__ __launch_bounds__(kNBlock) void k_nbr_rdf(NbrGridDev G, const double4* pos, const int* start, int n, RdfArgs A,
                                                     unsigned long long* acc)
{
  extern __shared__ unsigned int h[];
  const int nh = A.nbin * A.npairs;
  for (int b = threadIdx.x; b < nh; b += kNBlock) h[b] = 0u;
  __syncthreads();
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  double4 me = make_double4(0.0, 0.0, 0.0, 0.0);
  if (p < n) me = pos[p];
  const int ti = nbr_type(me);
  const bool in = p < n && (nbr_mask(me) & A.groupbit) != 0;
  // the group atoms of each pair's type ranges: every lane of the wave is here, one lane adds the wave's count
  for (int m = 0; m < A.npairs; m++) {
    const int4 r = A.pairs[m];
    const bool a = in && ti >= r.x && ti <= r.y, b = in && ti >= r.z && ti <= r.w;
    const int ca = __popcll(__ballot(a)), cb = __popcll(__ballot(b)), cd = __popcll(__ballot(a && b));
    if (lane == 0) {
      unsigned long long* cnt = acc + nh + 3 * m;
      if (ca) atomicAdd(&cnt[0], (unsigned long long)ca);
      if (cb) atomicAdd(&cnt[1], (unsigned long long)cb);
      if (cd) atomicAdd(&cnt[2], (unsigned long long)cd);
    }
  }
  if (in) {
    int cx, cy, cz;
    nbr_cell(G, me.x, me.y, me.z, &cx, &cy, &cz);
    nbr_walk(G, pos, start, p, me, cx, cy, cz, [&](const double4& o, double rsq) {
      if (rsq > A.rsq_skip || !(nbr_mask(o) & A.groupbit)) return;
      const double q = sqrt_rn(rsq) * A.delrinv;
      if (!(q < (double)A.nbin)) return;   // (ibin >= Nbin: skipped)
      const int ibin = (int)q;
      const int tj = nbr_type(o);
      for (int m = 0; m < A.npairs; m++) {
        const int4 r = A.pairs[m];
        const bool counted = ti >= r.x && ti <= r.y && tj >= r.z && tj <= r.w;
        // the lanes that are at this place of the walk together: where all that count share one bin, 64 lanes would hit one
        // LDS address, and the first of them adds for all
        const unsigned long long mk = __ballot(counted);
        if (mk) {
          const int first = __ffsll((long long)mk) - 1;
          const int b0 = __shfl(ibin, first, 64);
          if (__ballot(counted && ibin != b0) == 0ull) {
            if (lane == first) atomicAdd(&h[m * A.nbin + b0], (unsigned int)__popcll(mk));
          } else if (counted)
            atomicAdd(&h[m * A.nbin + ibin], 1u);
        }
      }
    });
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nh; b += kNBlock) {
    const unsigned int k = h[b];
    if (k) atomicAdd(&acc[b], (unsigned long long)k);
  }
}

// out: [nbin][1 + 2 npairs] row-major.  One lane per pair; the running ncoord makes the bins of a pair sequential
__global__ __launch_bounds__(64) void k_rdf_norm(const unsigned long long* acc, int nbin, int npairs, double delr, double constant,
                                                 double* out)
{
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= npairs) return;
  const int nh = nbin * npairs, ncols = 1 + 2 * npairs;
  const unsigned long long ic = acc[nh + 3 * m], jc = acc[nh + 3 * m + 1], dup = acc[nh + 3 * m + 2];
  const double icount = (double)ic;
  const double normfac = ic > 0 ? (double)jc - (double)dup / icount : 0.0;
  double ncoord = 0.0;
  for (int ibin = 0; ibin < nbin; ibin++) {
    const double rlower = (double)ibin * delr, rupper = (double)(ibin + 1) * delr;
    const double vfrac = constant * (rupper * rupper * rupper - rlower * rlower * rlower);
    const double vn = vfrac * normfac;
    const double gr = vn != 0.0 ? (double)acc[(size_t)m * nbin + ibin] / (vn * icount) : 0.0;
    if (ic != 0) ncoord += gr * vfrac * normfac;
    double* row = out + (size_t)ibin * ncols;
    if (m == 0) row[0] = ((double)ibin + 0.5) * delr;
    row[1 + 2 * m] = gr;
    row[2 + 2 * m] = ncoord;
  }
}

struct CoordArgs {
  int nr, groupbit;
  double rcsq;
  int lo[kCoordMaxRanges], hi[kCoordMaxRanges];
};

__global__ __launch_bounds__(kNBlock) void k_nbr_coord(NbrGridDev G, const double4* pos, const int* start, const int* idx, int n,
                                                       CoordArgs A, double* val)
{
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  if (p >= n) return;
  const double4 me = pos[p];
  int cnt[kCoordMaxRanges];
#pragma unroll
  for (int k = 0; k < kCoordMaxRanges; k++) cnt[k] = 0;
  if (nbr_mask(me) & A.groupbit) {
    int cx, cy, cz;
    nbr_cell(G, me.x, me.y, me.z, &cx, &cy, &cz);
    nbr_walk(G, pos, start, p, me, cx, cy, cz, [&](const double4& o, double rsq) {
      if (!(rsq < A.rcsq)) return;
      const int tj = nbr_type(o);
#pragma unroll
      for (int k = 0; k < kCoordMaxRanges; k++)
        if (k < A.nr) cnt[k] += tj >= A.lo[k] && tj <= A.hi[k] ? 1 : 0;
    });
  }
  const int i = idx[p];
#pragma unroll
  for (int k = 0; k < kCoordMaxRanges; k++)
    if (k < A.nr) val[(size_t)k * (size_t)n + i] = (double)cnt[k];
}

// ---- compute cluster/atom: connected components over the places of the cell order ----
//
// parent[p] is a place of the same component with parent[p] <= p, or -1 for a place outside the group, which is never read as a
// neighbour and never hooked.  What may be assumed about memory inside one launch: NOTHING about plain stores of other
// workgroups (the L2s of the XCDs are not coherent and a CU's L1 is never refreshed).  So inside a launch `parent` is read and
// written with agent-scope integer atomics alone, as k_nbr_keys does with `count`, and everything else (the records, the radii,
// the flag's zero, mintag, cnt, val) is handed over at kernel boundaries.  And no result rests even on an atomic load being
// fresh: a value of parent[q] that is out of date is an OLDER ANCESTOR of q in the same tree (an entry only ever moves from q
// to an ancestor of q: a root is hooked once, under a smaller place, by a compare-and-swap that fails when it is no root any
// more; halving and compressing replace a parent by a grandparent or the root), so whatever a load returns, a root-finding
// loop walks a strictly decreasing chain inside q's tree and ends after at most n steps, and two places found under one place
// ARE in one tree.  That the hooks are complete is not taken on trust either: the verify launch reads only what earlier
// launches wrote unless it hooks something itself, and then it raises the flag and the host runs it again.
struct ClusterArgs {
  int groupbit, surface;
  double cut, cutsq;
};

// The link rule.  Bit-symmetric in (i, j), which the walk relies on when it takes every edge from its higher place alone:
// d = xj - xi and xi - xj are exact negations of each other, the two branches of the minimum image mirror each other, so rsq
// has the same bits from both ends; ri + rj is commutative.  surface: [own] the reach test of fix cohesive with cut for smax,
// each operation rounded once
__device__ __forceinline__ bool cl_linked(const ClusterArgs& A, double rsq, double ri, double rj)
{
  if (A.surface) {
    const double s = (ri + rj) + A.cut;
    return rsq < s * s;
  }
  return rsq < A.cutsq;
}

__device__ __forceinline__ int cl_load(const int* parent, int q)
{
  return __hip_atomic_load(parent + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above q as far as this lane can see: parent[r] < r on every step, so at most q + 1 of them.  HALVE: an entry on
// the way is lowered to its grandparent (an atomic minimum: the entry never rises, and a root is left alone)
template <bool HALVE>
__device__ __forceinline__ int cl_find(int* parent, int q)
{
  for (;;) {
    const int r = cl_load(parent, q);
    if (r == q) return q;
    const int g = cl_load(parent, r);
    if (g == r) return r;
    if (HALVE) atomicMin(&parent[q], g);
    q = g;
  }
}

// the trees of a and b become one; true where this lane hooked a root.  A root `hi` goes under the smaller place `lo` (a root
// or not: lo < hi keeps parent[q] <= q) only while it still is a root; where another lane was first, its new parent `old` is
// an ancestor of hi below hi, and the loop goes on with (old, lo): max(a, b) falls with every turn
template <bool HALVE>
__device__ __forceinline__ bool cl_unite(int* parent, int a, int b)
{
  for (;;) {
    a = cl_find<HALVE>(parent, a);
    b = cl_find<HALVE>(parent, b);
    if (a == b) return false;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return true;
    a = old;
    b = lo;
  }
}

// mintag and cnt are per place and used at the roots
__global__ __launch_bounds__(kNBlock) void k_cl_init(const double4* pos, int n, int groupbit, int* parent, int* mintag, int* cnt)
{
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  if (p >= n) return;
  parent[p] = (nbr_mask(pos[p]) & groupbit) ? p : -1;
  mintag[p] = INT_MAX;
  cnt[p] = 0;
}

// surface yes: the radii in cell order, next to the 32-byte records that rdf and coord/atom read
__global__ __launch_bounds__(kNBlock) void k_cl_pack_radius(const double4* xr, const int* idx, int n, double* rad)
{
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  if (p < n) rad[p] = xr[idx[p]].w;
}

// One lane per place p of the group: every linked neighbour at a place j < p (each edge once, from its higher end; the record
// and the radius of j are one broadcast line each for the lanes of a cell).  VERIFY = false, the hook launch: the two trees
// are united.  VERIFY = true, a launch of its own behind a compress: the same, without halving, so that a launch in which
// every pair is found under one root has written nothing and has read only what earlier launches wrote; a pair that is not
// is hooked and raises the flag
template <bool VERIFY>
__global__ __launch_bounds__(kNBlock) void k_cl_edges(NbrGridDev G, const double4* pos, const int* start, const double* rad, int n,
                                                      ClusterArgs A, int* parent, int* flag)
{
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  if (p >= n) return;
  const double4 me = pos[p];
  if (!(nbr_mask(me) & A.groupbit)) return;
  const double ri = A.surface ? rad[p] : 0.0;
  int cx, cy, cz;
  nbr_cell(G, me.x, me.y, me.z, &cx, &cy, &cz);
  bool raised = false;
  nbr_walk_places(G, pos, start, p, me, cx, cy, cz, [&](int j, const double4& o, double rsq) {
    if (j > p || !(nbr_mask(o) & A.groupbit)) return;
    const double rj = A.surface ? rad[j] : 0.0;
    if (!cl_linked(A, rsq, ri, rj)) return;
    if (cl_unite<!VERIFY>(parent, p, j)) raised = true;
  });
  if (VERIFY && raised) atomicOr(flag, 1);
}

// parent[p] becomes the root above p in the array as the launch before left it: no root moves in this launch, and an entry
// another lane has stored already is that lane's root, which is this one's too.  Place 0 zeroes the flag of the verify launch
// that follows (handed over by the kernel boundary)
__global__ __launch_bounds__(kNBlock) void k_cl_compress(int* parent, int n, int* flag)
{
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  if (p >= n) return;
  if (p == 0) *flag = 0;
  const int q = cl_load(parent, p);
  if (q < 0) return;
  const int r = cl_find<false>(parent, q);
  if (r != q) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// behind a verify launch that raised nothing: parent[p] is the root.  Integer atomics: the order changes no bit
__global__ __launch_bounds__(kNBlock) void k_cl_tally(const int* parent, const int* idx, const int* tag, int n, int size,
                                                      int* mintag, int* cnt)
{
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  if (p >= n) return;
  const int r = parent[p];
  if (r < 0) return;
  atomicMin(&mintag[r], tag[idx[p]]);
  if (size) atomicAdd(&cnt[r], 1);
}

__global__ __launch_bounds__(kNBlock) void k_cl_store(const int* parent, const int* idx, int n, int size, const int* mintag,
                                                      const int* cnt, double* val)
{
  const int p = blockIdx.x * kNBlock + threadIdx.x;
  if (p >= n) return;
  const int r = parent[p], i = idx[p];
  val[i] = r < 0 ? 0.0 : (double)mintag[r];
  if (size) val[(size_t)n + i] = r < 0 ? 0.0 : (double)cnt[r];
}

// ---- host side ----

struct RawTmp {   // the scratch of the sort and scan wrappers of sf_sort.hip, which grow it themselves
  void* p = nullptr;
  size_t n = 0;
  ~RawTmp()
  {
    if (p) (void)hipFree(p);
  }
};

struct NbrGrid {
  double rc = 0.0;
  NbrGridDev D{};
  int ncells = 1;
  DeviceScratch key_in, idx_in, key_out, idx_out, count, start, pos;
  DeviceScratch rad;   // the radii in cell order: made when a compute cluster/atom with surface yes asks, never otherwise
  RawTmp sort_tmp, scan_tmp;
  StateStamp made, rad_made;   // what it (and rad) was made at
};

struct RdfCompute {
  std::string id;
  int groupbit = 1;
  RdfSpec S;
  double delr = 0.0, delrinv = 0.0;
  int4* d_pairs = nullptr;
  unsigned long long* d_acc = nullptr;   // [npairs * nbin + 3 * npairs]
  double* d_out = nullptr;               // [nbin][1 + 2 npairs]
  StateStamp made;
  int npairs() const { return (int)S.pairs.size(); }
  int ncols() const { return 1 + 2 * npairs(); }
  size_t nacc() const { return (size_t)npairs() * (size_t)S.nbin + 3 * (size_t)npairs(); }
  ~RdfCompute()
  {
    if (d_pairs) (void)hipFree(d_pairs);
    if (d_acc) (void)hipFree(d_acc);
    if (d_out) (void)hipFree(d_out);
  }
};

constexpr size_t kMaxGrids = 4;   // distinct cutoffs kept at once

struct NbrSet {
  std::vector<std::unique_ptr<RdfCompute>> computes;
  std::vector<std::unique_ptr<NbrGrid>> grids;
  DeviceScratch cost_val;   // sf_lammps_nbr_cost of a compute coord/atom: where its columns go
  long long grid_builds = 0, launches = 0, host_copies = 0;
  RdfCompute* find(const std::string& id)
  {
    for (auto& c : computes)
      if (c->id == id) return c.get();
    return nullptr;
  }
};

NbrSet* set_of(const SfLammps& L) { return L.nbr.get<NbrSet>(); }
NbrSet& ensure_set(SfLammps& L) { return L.nbr.ensure<NbrSet>(); }

// The cells of cutoff rc over the box as it is now: at least rc (1 + 2^-20) wide, so that the rounding of a cell index
// (2^-52 of it) cannot put two atoms closer than rc into cells that are not adjacent; at most 2 n + 64 of them (a box that is
// mostly empty gets wider cells).  Refuses a periodic dimension shorter than 2 rc, where the minimum image is not unique
NbrGridDev make_cells(const SfLammps& L, const char* who, double rc, int* ncells)
{
  double lo[3], hi[3];
  int per[3];
  L.eng.box(lo, hi, per);
  NbrGridDev D{};
  const double edge = rc * (1.0 + 0x1p-20);
  for (int a = 0; a < 3; a++) {
    const double len = hi[a] - lo[a];
    if (per[a] && len < 2.0 * rc)
      fail("%s: cutoff is longer than half a periodic box length (%g against %g in dimension %c)", who, rc, len, "xyz"[a]);
    D.lo[a] = lo[a];
    D.prd[a] = len;
    D.half[a] = 0.5 * len;
    D.periodic[a] = per[a];
    const double q = len > 0.0 ? std::floor(len / edge) : 1.0;
    D.nc[a] = (int)std::min(std::max(q, 1.0), 1048576.0);
  }
  const double cap = 2.0 * (double)L.eng.nlocal() + 64.0;
  double prod = (double)D.nc[0] * D.nc[1] * D.nc[2];
  if (prod > cap) {
    const double f = std::cbrt(cap / prod);
    for (int a = 0; a < 3; a++) D.nc[a] = std::max(1, (int)std::floor(D.nc[a] * f));
  }
  while ((double)D.nc[0] * D.nc[1] * D.nc[2] > cap) {   // (the floor of one count and the 1 of another can leave it above)
    int a = 0;
    for (int b = 1; b < 3; b++)
      if (D.nc[b] > D.nc[a]) a = b;
    D.nc[a]--;
  }
  for (int a = 0; a < 3; a++) {
    D.inv[a] = D.prd[a] > 0.0 ? (double)D.nc[a] / D.prd[a] : 0.0;
    const bool wrap = D.periodic[a] != 0;
    // one cell: itself; two: both, each once (a periodic -1 and +1 are the same cell); else the three
    D.noff[a] = D.nc[a] == 1 ? 1 : (D.nc[a] == 2 && wrap ? 2 : 3);
    D.off0[a] = D.noff[a] == 3 ? -1 : 0;
  }
  *ncells = D.nc[0] * D.nc[1] * D.nc[2];
  return D;
}

void build_grid(SfLammps& L, NbrSet& T, NbrGrid& g, const NbrGridDev& D, int ncells)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int n = e.nlocal();
  const size_t m = (size_t)std::max(n, 1);
  g.D = D;
  g.ncells = ncells;
  unsigned* key_in = static_cast<unsigned*>(g.key_in.get(sizeof(unsigned) * m, st));
  int* idx_in = static_cast<int*>(g.idx_in.get(sizeof(int) * m, st));
  unsigned* key_out = static_cast<unsigned*>(g.key_out.get(sizeof(unsigned) * m, st));
  int* idx_out = static_cast<int*>(g.idx_out.get(sizeof(int) * m, st));
  int* count = static_cast<int*>(g.count.get(sizeof(int) * ((size_t)ncells + 4), st));
  int* start = static_cast<int*>(g.start.get(sizeof(int) * ((size_t)ncells + 4), st));
  double4* pos = static_cast<double4*>(g.pos.get(sizeof(double4) * m, st));
  SF_HIP(hipMemsetAsync(count, 0, sizeof(int) * ((size_t)ncells + 1), st));
  if (n > 0) {
    k_nbr_keys<<<div_up(n, kNBlock), kNBlock, 0, st>>>(D, e.d_xr(), n, key_in, idx_in, count);
    SF_HIP(hipGetLastError());
  }
  exclusive_scan_i32(g.scan_tmp.p, g.scan_tmp.n, count, start, ncells + 1, st);   // (start[ncells] = n)
  if (n > 0) {
    int keybits = 1;
    while (keybits < 32 && (1ll << keybits) < (long long)ncells) keybits++;
    sort_pairs_u32(g.sort_tmp.p, g.sort_tmp.n, key_in, key_out, idx_in, idx_out, n, keybits, st);
    k_nbr_pack<<<div_up(n, kNBlock), kNBlock, 0, st>>>(e.d_xr(), e.d_type(), e.d_mask(), idx_out, n, pos);
    SF_HIP(hipGetLastError());
    T.launches += 3;   // (the sort counts as one)
  }
  T.launches++;
  T.grid_builds++;
  g.made.set(e);
  g.rad_made.clear();
}

// the grid of cutoff rc on the state as it stands: kept with the step, the rebuild count, the atom count and the cell
// dimensions it was made at, and shared by every compute of that cutoff
NbrGrid& grid_of(SfLammps& L, NbrSet& T, const char* who, double rc, bool force = false)
{
  int ncells = 1;
  const NbrGridDev D = make_cells(L, who, rc, &ncells);
  NbrGrid* g = nullptr;
  for (auto& q : T.grids)
    if (q->rc == rc) g = q.get();
  if (!g) {
    if (T.grids.size() >= kMaxGrids) {
      SF_HIP(hipStreamSynchronize(L.eng.stream()));   // (a walk queued on the stream may still read it)
      T.grids.erase(T.grids.begin());
    }
    T.grids.push_back(std::make_unique<NbrGrid>());
    g = T.grids.back().get();
    g->rc = rc;
  }
  const bool same = g->made.is_now(L.eng) && std::memcmp(&g->D, &D, sizeof(D)) == 0;
  if (!same || force) build_grid(L, T, *g, D, ncells);
  return *g;
}

void rdf_walk(SfLammps& L, NbrSet& T, RdfCompute& c, const NbrGrid& g)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int n = e.nlocal();
  SF_HIP(hipMemsetAsync(c.d_acc, 0, sizeof(unsigned long long) * c.nacc(), st));
  if (n > 0) {
    const RdfArgs A{(int)c.S.nbin, c.npairs(), c.groupbit, c.delrinv, c.S.rc * c.S.rc * (1.0 + 1.0e-9), c.d_pairs};
    const size_t lds = sizeof(unsigned int) * (size_t)c.S.nbin * (size_t)c.npairs();
    k_nbr_rdf<<<div_up(n, kNBlock), kNBlock, lds, st>>>(g.D, g.pos.as<double4>(), g.start.as<int>(), n, A, c.d_acc);
    T.launches++;
  }
  const double constant = 4.0 * 3.14159265358979323846 / (3.0 * g.D.prd[0] * g.D.prd[1] * g.D.prd[2]);
  k_rdf_norm<<<div_up(c.npairs(), 64), 64, 0, st>>>(c.d_acc, (int)c.S.nbin, c.npairs(), c.delr, constant, c.d_out);
  SF_HIP(hipGetLastError());
  T.launches++;
}

void rdf_evaluate(SfLammps& L, NbrSet& T, RdfCompute& c)
{
  nbr_refuse_unsupported(L, "compute rdf");
  if (c.made.is_now(L.eng)) {
    int ncells = 1;
    (void)make_cells(L, "compute rdf", c.S.rc, &ncells);   // (the box check, also where the values are fresh)
    return;
  }
  rdf_walk(L, T, c, grid_of(L, T, "compute rdf", c.S.rc));
  c.made.set(L.eng);
}

CoordArgs coord_args(int groupbit, double rc, const std::vector<TypeRange>& ranges)
{
  CoordArgs A{};
  A.nr = (int)ranges.size();
  A.groupbit = groupbit;
  A.rcsq = rc * rc;
  for (int k = 0; k < A.nr; k++) {
    A.lo[k] = ranges[k].lo;
    A.hi[k] = ranges[k].hi;
  }
  return A;
}

void coord_walk(SfLammps& L, NbrSet& T, const NbrGrid& g, const CoordArgs& A, double* val)
{
  const int n = L.eng.nlocal();
  if (n <= 0) return;
  k_nbr_coord<<<div_up(n, kNBlock), kNBlock, 0, L.eng.stream()>>>(g.D, g.pos.as<double4>(), g.start.as<int>(), g.idx_out.as<int>(),
                                                                  n, A, val);
  SF_HIP(hipGetLastError());
  T.launches++;
}

constexpr int kClusterMaxRounds = 64;

// init, hook, then compress + verify until a verify launch raises nothing (one 4-byte copy per round), tally, store
void cluster_walk(SfLammps& L, NbrSet& T, NbrGrid& g, const char* who, int groupbit, const ClusterSpec& S, ClusterWork& W,
                  double* val)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int n = e.nlocal();
  W.rounds = 0;
  if (n <= 0) return;
  const size_t m = (size_t)n;
  int* parent = static_cast<int*>(W.buf.get(sizeof(int) * (3 * m + 4), st));
  int *mintag = parent + m, *cnt = mintag + m, *flag = cnt + m;
  const unsigned nb = (unsigned)div_up(n, kNBlock);
  const double4* pos = g.pos.as<double4>();
  const int *start = g.start.as<int>(), *idx = g.idx_out.as<int>();
  const double* rad = nullptr;
  if (S.surface) {
    double* r = static_cast<double*>(g.rad.get(sizeof(double) * m, st));
    if (!g.rad_made.is_now(e)) {
      k_cl_pack_radius<<<nb, kNBlock, 0, st>>>(e.d_xr(), idx, n, r);
      SF_HIP(hipGetLastError());
      T.launches++;
      g.rad_made.set(e);
    }
    rad = r;
  }
  const ClusterArgs A{groupbit, S.surface ? 1 : 0, S.cut, S.cut * S.cut};
  k_cl_init<<<nb, kNBlock, 0, st>>>(pos, n, groupbit, parent, mintag, cnt);
  k_cl_edges<false><<<nb, kNBlock, 0, st>>>(g.D, pos, start, rad, n, A, parent, flag);
  SF_HIP(hipGetLastError());
  T.launches += 2;
  for (;;) {
    k_cl_compress<<<nb, kNBlock, 0, st>>>(parent, n, flag);
    k_cl_edges<true><<<nb, kNBlock, 0, st>>>(g.D, pos, start, rad, n, A, parent, flag);
    SF_HIP(hipGetLastError());
    T.launches += 2;
    int raised = 0;
    SF_HIP(hipMemcpyAsync(&raised, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    T.host_copies++;
    W.rounds++;
    if (!raised) break;
    if (W.rounds >= kClusterMaxRounds) fail("%s: the components did not settle within %d verify rounds", who, W.rounds);
  }
  k_cl_tally<<<nb, kNBlock, 0, st>>>(parent, idx, e.d_tag(), n, S.size ? 1 : 0, mintag, cnt);
  k_cl_store<<<nb, kNBlock, 0, st>>>(parent, idx, n, S.size ? 1 : 0, mintag, cnt, val);
  SF_HIP(hipGetLastError());
  T.launches += 2;
}

RdfCompute& rdf_of(SfLammps& L, const std::string& id)
{
  NbrSet* T = set_of(L);
  RdfCompute* c = T ? T->find(id) : nullptr;
  if (!c) fail("Could not find compute ID %s", id.c_str());
  return *c;
}

// ---- the kind (sf_compute_ids.h) ----

bool is_style(const std::string& style) { return style == "rdf"; }

void define(SfLammps& L, const std::vector<std::string>& w)
{
  auto c = std::make_unique<RdfCompute>();
  c->id = w[1];
  c->groupbit = L.eng.group_bit(w[2]);
  nbr_refuse_unsupported(L, "compute rdf");
  const std::string err = parse_rdf(w, &c->S);
  if (!err.empty()) fail("%s", err.c_str());
  c->delr = c->S.rc / (double)c->S.nbin;
  c->delrinv = 1.0 / c->delr;
  hipStream_t st = L.eng.stream();
  std::vector<int4> pairs;
  for (const RdfPair& p : c->S.pairs) pairs.push_back(make_int4(p.i.lo, p.i.hi, p.j.lo, p.j.hi));
  SF_HIP(hipMalloc(&c->d_pairs, sizeof(int4) * pairs.size()));
  SF_HIP(hipMalloc(&c->d_acc, sizeof(unsigned long long) * c->nacc()));
  SF_HIP(hipMalloc(&c->d_out, sizeof(double) * (size_t)c->S.nbin * (size_t)c->ncols()));
  SF_HIP(hipMemcpyAsync(c->d_pairs, pairs.data(), sizeof(int4) * pairs.size(), hipMemcpyHostToDevice, st));
  SF_HIP(hipMemsetAsync(c->d_out, 0, sizeof(double) * (size_t)c->S.nbin * (size_t)c->ncols(), st));
  SF_HIP(hipStreamSynchronize(st));   // (`pairs` is pageable and leaves scope)
  ensure_set(L).computes.push_back(std::move(c));
}

bool shape(const SfLammps& L, const std::string& id, ComputeShape* s)
{
  NbrSet* T = set_of(L);
  const RdfCompute* c = T ? T->find(id) : nullptr;
  if (!c) return false;
  *s = ComputeShape();
  s->kind = CK_ARRAY;
  s->n = c->ncols();
  s->rows = (int)c->S.nbin;
  return true;
}

void remove(SfLammps& L, const std::string& id)
{
  if (NbrSet* T = set_of(L)) compute_take(L, T->computes, id);   // (a launch queued on the stream may still write its values)
}

// (and the grids, which the walks of compute coord/atom share)
void invalidate(SfLammps& L)
{
  if (NbrSet* T = set_of(L)) {
    for (auto& c : T->computes) c->made.clear();
    for (auto& g : T->grids) g->made.clear(), g->rad_made.clear();
  }
}

}  // namespace

void nbr_refuse_unsupported(const SfLammps& L, const char* who) { refuse_decomposed(L, who); }

const ComputeKindOps& rdf_compute_kind()
{
  static const ComputeKindOps kind = {is_style, define, remove, shape, invalidate};
  return kind;
}

const double* rdf_array_device(SfLammps& L, const std::string& id)
{
  RdfCompute& c = rdf_of(L, id);
  rdf_evaluate(L, *set_of(L), c);
  return c.d_out;
}

void nbr_coord_atom(SfLammps& L, const char* who, int groupbit, double rc, const std::vector<TypeRange>& ranges, double* val)
{
  nbr_refuse_unsupported(L, who);
  NbrSet& T = ensure_set(L);
  const NbrGrid& g = grid_of(L, T, who, rc);
  coord_walk(L, T, g, coord_args(groupbit, rc, ranges), val);
}

double nbr_cluster_grid_cutoff(SfLammps& L, const ClusterSpec& S)
{
  // (the engine's largest radius, max_radius(): one rank here, so the local one is it)
  return S.surface ? 2.0 * L.eng.local_max_radius() + S.cut : S.cut;
}

void nbr_cluster_atom(SfLammps& L, const char* who, int groupbit, const ClusterSpec& S, ClusterWork& W, double* val)
{
  nbr_refuse_unsupported(L, who);
  NbrSet& T = ensure_set(L);
  NbrGrid& g = grid_of(L, T, who, nbr_cluster_grid_cutoff(L, S));
  cluster_walk(L, T, g, who, groupbit, S, W, val);
}

}  // namespace sf

using sf::handle;

extern "C" {

long long sf_lammps_compute_array(void* ptr, const char* id, long long max, double* values, int* ncols)
{
  long long n = 0;
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id) sf::fail("sf_lammps_compute_array: null argument");
  if (sf::pchunk_holds(L, id)) {   // (a per-chunk compute: Nchunk rows, known once its chunk/atom compute is evaluated)
    int rows = 0, nc = 0;
    const double* d = sf::pchunk_array_device(L, id, &rows, &nc);
    if (ncols) *ncols = nc;
    n = (long long)rows * nc;
    if (n > 0 && n <= max) {
      if (!values) sf::fail("sf_lammps_compute_array: null argument");
      hipStream_t st = L.eng.stream();
      SF_HIP(hipMemcpyAsync(values, d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
      SF_HIP(hipStreamSynchronize(st));
    }
    return n;
  }
  const sf::ComputeShape shape = sf::compute_shape(L, id);
  sf::fail_if(sf::check_get_array(shape, id));
  if (ncols) *ncols = shape.n;
  n = (long long)shape.rows * shape.n;
  if (n <= max) {
    if (!values) sf::fail("sf_lammps_compute_array: null argument");
    const double* d = sf::rdf_array_device(L, id);
    hipStream_t st = L.eng.stream();
    SF_HIP(hipMemcpyAsync(values, d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    sf::set_of(L)->host_copies++;
  }
  SF_API_END(n)
}

// counts: [npairs][nbin]; per_pair: icount jcount duplicates of each pair, [npairs][3].  Returns npairs * nbin
long long sf_lammps_rdf_counts(void* ptr, const char* id, long long max, long long* counts, long long* per_pair, int* npairs)
{
  long long n = 0;
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id) sf::fail("sf_lammps_rdf_counts: null argument");
  sf::NbrSet* T = sf::set_of(L);
  sf::RdfCompute* found = T ? T->find(id) : nullptr;
  if (!found) sf::fail("Could not find compute rdf ID %s", id);
  sf::RdfCompute& c = *found;
  if (npairs) *npairs = c.npairs();
  n = (long long)c.npairs() * c.S.nbin;
  if (n <= max) {
    if (!counts || !per_pair) sf::fail("sf_lammps_rdf_counts: null argument");
    sf::rdf_evaluate(L, *sf::set_of(L), c);
    hipStream_t st = L.eng.stream();
    static_assert(sizeof(long long) == sizeof(unsigned long long), "counter width");
    SF_HIP(hipMemcpyAsync(counts, c.d_acc, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(per_pair, c.d_acc + n, sizeof(long long) * 3 * (size_t)c.npairs(), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    sf::set_of(L)->host_copies++;
  }
  SF_API_END(n)
}

int sf_lammps_nbr_launches(void* ptr, long long* grid_builds, long long* launches, long long* host_copies)
{
  SF_API_BEGIN
  if (!grid_builds || !launches || !host_copies) sf::fail("sf_lammps_nbr_launches: null argument");
  const sf::NbrSet* T = sf::set_of(*handle(ptr));
  *grid_builds = T ? T->grid_builds : 0;
  *launches = T ? T->launches : 0;
  *host_copies = T ? T->host_copies : 0;
  SF_API_END(0)
}

// the verify rounds of the last evaluation of compute cluster/atom `id` (0: not evaluated yet, or no atoms)
int sf_lammps_cluster_rounds(void* ptr, const char* id, int* rounds)
{
  SF_API_BEGIN
  if (!id || !rounds) sf::fail("sf_lammps_cluster_rounds: null argument");
  const sf::ClusterWork* W = sf::atom_compute_cluster_spec(*handle(ptr), id, nullptr, nullptr);
  if (!W) sf::fail("Could not find compute cluster/atom ID %s", id);
  *rounds = W->rounds;
  SF_API_END(0)
}

// GPU milliseconds from HIP events of one fresh grid build and one walk of compute `id` (rdf, coord/atom or cluster/atom: its
// walk is everything after the grid, the waits for the flag of the verify rounds included)
int sf_lammps_nbr_cost(void* ptr, const char* id, double* grid_ms, double* walk_ms)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id || !grid_ms || !walk_ms) sf::fail("sf_lammps_nbr_cost: null argument");
  hipStream_t st = L.eng.stream();
  sf::NbrSet& T = sf::ensure_set(L);
  int cl_groupbit = 1;
  sf::ClusterSpec cl;
  if (sf::RdfCompute* c = T.find(id)) {
    sf::nbr_refuse_unsupported(L, "compute rdf");
    sf::NbrGrid* g = nullptr;
    *grid_ms = sf::stream_ms(st, [&] { g = &sf::grid_of(L, T, "compute rdf", c->S.rc, true); });
    *walk_ms = sf::stream_ms(st, [&] { sf::rdf_walk(L, T, *c, *g); });
    c->made.set(L.eng);
  } else if (sf::ClusterWork* W = sf::atom_compute_cluster_spec(L, id, &cl_groupbit, &cl)) {
    const char* who = "compute cluster/atom";
    sf::nbr_refuse_unsupported(L, who);
    const size_t cells = (cl.size ? 2 : 1) * (size_t)std::max(L.eng.nlocal(), 1);
    double* val = static_cast<double*>(T.cost_val.get(sizeof(double) * cells, st));   // (not in the time)
    sf::NbrGrid* g = nullptr;
    *grid_ms = sf::stream_ms(st, [&] { g = &sf::grid_of(L, T, who, sf::nbr_cluster_grid_cutoff(L, cl), true); });
    *walk_ms = sf::stream_ms(st, [&] { sf::cluster_walk(L, T, *g, who, cl_groupbit, cl, *W, val); });   // (everything after the grid)
  } else {
    int groupbit = 1;
    double rc = 0.0;
    std::vector<sf::TypeRange> ranges;
    if (!sf::atom_compute_coord_spec(L, id, &groupbit, &rc, &ranges)) sf::fail("Could not find compute rdf or coord/atom ID %s", id);
    sf::nbr_refuse_unsupported(L, "compute coord/atom");
    const size_t cells = ranges.size() * (size_t)std::max(L.eng.nlocal(), 1);
    double* val = static_cast<double*>(T.cost_val.get(sizeof(double) * cells, st));   // (not in the time)
    sf::NbrGrid* g = nullptr;
    *grid_ms = sf::stream_ms(st, [&] { g = &sf::grid_of(L, T, "compute coord/atom", rc, true); });
    *walk_ms = sf::stream_ms(st, [&] { sf::coord_walk(L, T, *g, sf::coord_args(groupbit, rc, ranges), val); });
  }
  SF_API_END(0)
}

}  // extern "C"
