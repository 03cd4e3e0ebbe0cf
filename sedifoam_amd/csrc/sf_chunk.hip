// sf_chunk.hip -- binned profiles ([3P] LAMMPS names and rules):
//   compute ID group chunk/atom bin/1d|bin/2d|bin/3d dim origin delta [...] units box|reduced [bound dim lo hi] [discard ..]
//       one column, the chunk ID 1 + ((i1 n2) + i2) n3 + i3 of the layers an atom's coordinates fall in; 0 outside the group
//       or discarded.  A per-atom compute like those of sf_compute_atom.hip (c_ID in dump custom, sf_lammps_compute_atom).
//   fix ID group ave/chunk Nevery Nrepeat Nfreq chunkID vx vy vz fx fy fz density/number density/mass c_ID c_ID[k] ...
//       per-chunk sums of per-atom values, averaged over Nrepeat samples and written once per Nfreq steps.
// A sample reads the state AT THE MOMENT OF THE OUTPUT, like a dump frame, and stores nothing back into the run.
//
// One sample, on the engine's stream:
//   k_chunk_assign   one lane per owned atom: chunk ID (double, the compute's column), sort key, atom index
//   radix sort       stable (key, index) pairs with ceil(log2(nchunk + 1)) key bits (sf_sort.hip): the atoms of a chunk stay
//                    in index order
//   k_chunk_bounds   start[k] = first sorted position with key >= k, by a search on the sorted keys
//   k_chunk_tiles    tiles of kTile atoms per chunk: the cut depends on the segment's length only; then an exclusive scan
//   k_chunk_sums     one block per tile and group of up to 8 columns: fixed shuffle tree in a wave, the four wave sums added
//                    in a fixed order; one partial per (column, tile)
//   k_chunk_fold     one lane per (column, chunk): the tile partials added IN TILE ORDER into the device accumulator
//                    [1 + nvalues][nchunk] (norm sample: divided by the sample's count first)
// No floating-point atomics anywhere: the same state in the same atom order gives the same bits.  The grouping (assign ..
// scan) is made once per step and shared by every fix that names the compute.  Nothing is copied to the host before the
// output step; there one copy, then normalisation, `ave running` and the text on the host in double.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_ave_fix.h"
#include "sf_chunk.h"
#include "sf_chunk_parse.h"
#include "sf_compute_atom.h"
#include "sf_compute_ids.h"
#include "sf_pchunk.h"
#include "sf_pchunk_parse.h"

namespace sf {
namespace {

constexpr int kTile = 256;      // atoms per reduction tile = lanes per block
constexpr int kColGroup = 8;    // columns one launch of k_chunk_sums reduces

__global__ __launch_bounds__(256) void k_chunk_assign(const double4* xr, const int* mask, int n, int groupbit, ChunkBins B,
                                                      double* val, unsigned* key, int* idx)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int id = 0;
  if (mask[i] & groupbit) {
    const double4 x = xr[i];
    int lin = 0;
    bool out = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (a < B.ndim) {
        const int d = B.dim[a];
        double c = d == 0 ? x.x : (d == 1 ? x.y : x.z);
        if (B.periodic[a]) {
          if (c < B.boxlo[a]) c += B.prd[a];
          if (c >= B.boxhi[a]) c -= B.prd[a];
        }
        int ibin = (int)((c - B.offset[a]) * B.invdelta[a]);
        if (c < B.offset[a]) ibin--;
        const int last = B.nlayers[a] - 1;
        if (ibin < 0) {
          out = out || B.discard[a];
          ibin = 0;
        } else if (ibin > last) {
          out = out || B.discard[a];
          ibin = last;
        }
        lin = lin * B.nlayers[a] + ibin;
      }
    }
    id = out ? 0 : 1 + lin;
  }
  val[i] = (double)id;
  key[i] = (unsigned)id;
  idx[i] = i;
}

// start[0 .. nchunk + 1]: start[k] = the first sorted position whose key is >= k (start[nchunk + 1] = n).  Every entry is
// written by exactly one lane: the one at the first position of the next key present
__global__ __launch_bounds__(256) void k_chunk_bounds(const unsigned* key, int n, int nchunk, int* start)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int k1 = min((int)key[p], nchunk);
  const int k0 = p == 0 ? 0 : min((int)key[p - 1], nchunk) + 1;
  for (int k = k0; k <= k1; k++) start[k] = p;
  if (p == n - 1)
    for (int k = k1 + 1; k <= nchunk + 1; k++) start[k] = n;
}

// ntile[c], c = 0 .. nchunk (chunk c + 1; the last entry is 0 so that the scan's last entry is the total)
__global__ __launch_bounds__(256) void k_chunk_tiles(const int* start, int nchunk, int* ntile)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > nchunk) return;
  ntile[c] = c < nchunk ? (start[c + 2] - start[c + 1] + kTile - 1) / kTile : 0;
}

enum Src { SRC_ONE, SRC_MASS, SRC_VX, SRC_VY, SRC_VZ, SRC_FX, SRC_FY, SRC_FZ, SRC_PTR };
struct ColGroup {
  int n;                         // columns in this launch
  int needv, needf;              // gather the velocity / force record
  int src[kColGroup];
  const double* p[kColGroup];    // SRC_PTR: a per-atom column indexed by atom
};

// one block per tile t of the sorted order; partial[q * pstride + t] = the tile's sum of column q
__global__ __launch_bounds__(kTile) void k_chunk_sums(const double4* vm, const double4* force, const int* mask, int groupbit,
                                                      const int* idx, const int* start, const int* tileoff, int nchunk,
                                                      ColGroup G, long long pstride, double* partial)
{
  __shared__ double ws[kColGroup][kTile / 64];
  const int t = blockIdx.x;
  if (t >= tileoff[nchunk]) return;   // (the grid is the upper bound n / kTile + nchunk; uniform over the block)
  // the chunk of tile t: the last c with tileoff[c] <= t (empty chunks share their successor's offset)
  int lo = 0, hi = nchunk;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tileoff[mid] <= t) lo = mid + 1;
    else hi = mid;
  }
  const int c = lo - 1;
  const int p = start[c + 1] + (t - tileoff[c]) * kTile + (int)threadIdx.x;
  bool in = p < start[c + 2];
  const int a = in ? idx[p] : 0;
  in = in && (mask[a] & groupbit);
  double4 v = make_double4(0.0, 0.0, 0.0, 0.0), f = v;
  if (in && G.needv) v = vm[a];
  if (in && G.needf) f = force[a];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kColGroup; q++) {
    if (q < G.n) {
      double s = 0.0;
      if (in) {
        switch (G.src[q]) {
          case SRC_ONE: s = 1.0; break;
          case SRC_MASS: s = v.w; break;
          case SRC_VX: s = v.x; break;
          case SRC_VY: s = v.y; break;
          case SRC_VZ: s = v.z; break;
          case SRC_FX: s = f.x; break;
          case SRC_FY: s = f.y; break;
          case SRC_FZ: s = f.z; break;
          default: s = G.p[q][a]; break;
        }
      }
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0) ws[q][w] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < G.n) {
    const int q = threadIdx.x;
    partial[(long long)q * pstride + t] = (ws[q][0] + ws[q][1]) + (ws[q][2] + ws[q][3]);
  }
}

// one lane per (column, chunk): the chunk's tile partials in tile order, added into the accumulator.  samplemask bit q:
// column q is divided by the sample's count (column 0) first -- norm sample; a sample with count 0 contributes 0
__global__ __launch_bounds__(256) void k_chunk_fold(const double* partial, long long pstride, const int* tileoff, int nchunk,
                                                    int ncol, unsigned samplemask, double* acc)
{
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e >= (long long)ncol * nchunk) return;
  const int q = (int)(e / nchunk), c = (int)(e % nchunk);
  const int t0 = tileoff[c], t1 = tileoff[c + 1];
  double s = 0.0;
  for (int t = t0; t < t1; t++) s += partial[(long long)q * pstride + t];
  if ((samplemask >> q) & 1u) {
    double cnt = 0.0;
    for (int t = t0; t < t1; t++) cnt += partial[t];
    s = cnt > 0.0 ? s / cnt : 0.0;
  }
  acc[e] += s;
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

struct ChunkCompute {
  std::string id;
  int groupbit = 1;
  ChunkBins B;
  int keybits = 1;
  DeviceScratch val, key_in, idx_in, key_out, idx_out, start, ntile, tileoff;
  RawTmp sort_tmp, scan_tmp;
  StateStamp assigned, grouped;   // what the assignment / the grouping was made at
};

struct AveFix : AveFixState {
  AveSpec S;
  int groupbit = 1;
  int nchunk = 0, ncol = 1;
  DeviceScratch partial, acc, cost_acc;
  std::vector<double> h_acc;
  // ave running: the sums of norm all (device layout) and the sums of the per-output results, over noutputs outputs
  std::vector<double> run_acc, run_res;
  long long noutputs = 0;
  std::vector<double> count, values;   // the latest output: [nchunk], row-major [nchunk][nvalues]
};

struct ChunkSet {
  std::vector<std::unique_ptr<ChunkCompute>> computes;
  std::vector<std::unique_ptr<AveFix>> fixes;
  long long launches = 0;
  ChunkCompute* find(const std::string& id)
  {
    for (auto& c : computes)
      if (c->id == id) return c.get();
    return nullptr;
  }
  AveFix* find_fix(const std::string& id) const { return ave_find(fixes, id); }
};

ChunkSet* set_of(const SfLammps& L) { return L.chunks.get<ChunkSet>(); }
ChunkSet& ensure_set(SfLammps& L) { return L.chunks.ensure<ChunkSet>(); }

void assign(SfLammps& L, ChunkSet& T, ChunkCompute& c)
{
  refuse_decomposed(L, "compute chunk/atom");
  DemEngine& e = L.eng;
  const int n = e.nlocal();
  hipStream_t st = e.stream();
  const size_t m = (size_t)std::max(n, 1);
  double* val = static_cast<double*>(c.val.get(sizeof(double) * m, st));
  unsigned* key = static_cast<unsigned*>(c.key_in.get(sizeof(unsigned) * m, st));
  int* idx = static_cast<int*>(c.idx_in.get(sizeof(int) * m, st));
  if (n > 0) {
    k_chunk_assign<<<div_up(n, 256), 256, 0, st>>>(e.d_xr(), e.d_mask(), n, c.groupbit, c.B, val, key, idx);
    SF_HIP(hipGetLastError());
    T.launches++;
  }
  c.assigned.set(e);
  c.grouped.clear();
}

// sort + bounds + tiles + scan of the assignment of this step (made first when it is stale)
void group_sorted(SfLammps& L, ChunkSet& T, ChunkCompute& c)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int n = e.nlocal(), nchunk = c.B.nchunk;
  const size_t m = (size_t)std::max(n, 1);
  unsigned* key_out = static_cast<unsigned*>(c.key_out.get(sizeof(unsigned) * m, st));
  int* idx_out = static_cast<int*>(c.idx_out.get(sizeof(int) * m, st));
  int* start = static_cast<int*>(c.start.get(sizeof(int) * ((size_t)nchunk + 2), st));
  int* ntile = static_cast<int*>(c.ntile.get(sizeof(int) * ((size_t)nchunk + 1), st));
  int* tileoff = static_cast<int*>(c.tileoff.get(sizeof(int) * ((size_t)nchunk + 1), st));
  if (n <= 0) return;
  sort_pairs_u32(c.sort_tmp.p, c.sort_tmp.n, c.key_in.as<unsigned>(), key_out, c.idx_in.as<int>(), idx_out, n, c.keybits, st);
  k_chunk_bounds<<<div_up(n, 256), 256, 0, st>>>(key_out, n, nchunk, start);
  k_chunk_tiles<<<div_up(nchunk + 1, 256), 256, 0, st>>>(start, nchunk, ntile);
  SF_HIP(hipGetLastError());
  exclusive_scan_i32(c.scan_tmp.p, c.scan_tmp.n, ntile, tileoff, nchunk + 1, st);
  T.launches += 4;   // (the sort and the scan count as one each)
}

void group(SfLammps& L, ChunkSet& T, ChunkCompute& c)
{
  if (!c.assigned.is_now(L.eng)) assign(L, T, c);
  else refuse_decomposed(L, "compute chunk/atom");
  if (c.grouped.is_now(L.eng)) return;
  group_sorted(L, T, c);
  c.grouped.set(L.eng);
}

Src src_of(int source)
{
  switch (source) {
    case AS_VX: return SRC_VX;
    case AS_VY: return SRC_VY;
    case AS_VZ: return SRC_VZ;
    case AS_FX: return SRC_FX;
    case AS_FY: return SRC_FY;
    case AS_FZ: return SRC_FZ;
    case AS_DENSITY_NUMBER: return SRC_ONE;
    case AS_DENSITY_MASS: return SRC_MASS;
    default: return SRC_PTR;
  }
}

bool per_atom_value(int source) { return source != AS_DENSITY_NUMBER && source != AS_DENSITY_MASS; }

// the column of a c_ value: checked at the fix line and again at every sample (the compute may have been redefined)
void check_compute_value(const SfLammps& L, const AveValue& v)
{
  fail_if(check_ave_chunk_value(compute_shape(L, v.id), v.index));
}

// the sums of one sample of fix F, added into acc (the fix's accumulator, or the scratch of the cost measurement)
void launch_sums(SfLammps& L, ChunkSet& T, AveFix& F, ChunkCompute& c, double* acc)
{
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int n = e.nlocal(), nchunk = c.B.nchunk;
  if (n <= 0) return;
  const int maxtiles = div_up(n, kTile) + nchunk;
  const int src0 = SRC_ONE;
  std::vector<int> src(1, src0);
  std::vector<const double*> ptr(1, nullptr);
  unsigned samplemask = 0;
  for (size_t j = 0; j < F.S.values.size(); j++) {
    const AveValue& v = F.S.values[j];
    const double* p = nullptr;
    if (v.source == AS_COMPUTE) {
      check_compute_value(L, v);
      int nc = 0;
      const double* val = atom_compute_values(L, v.id, &nc);   // (once per step however many ask)
      p = val + (size_t)(v.index > 0 ? v.index - 1 : 0) * (size_t)n;
    }
    src.push_back(src_of(v.source));
    ptr.push_back(p);
    if (F.S.norm == 1 && per_atom_value(v.source)) samplemask |= 1u << (j + 1);
  }
  double* partial = static_cast<double*>(F.partial.get(sizeof(double) * (size_t)F.ncol * (size_t)maxtiles, st));
  for (int col0 = 0; col0 < F.ncol; col0 += kColGroup) {
    ColGroup G{};
    G.n = std::min(kColGroup, F.ncol - col0);
    for (int q = 0; q < G.n; q++) {
      G.src[q] = src[col0 + q];
      G.p[q] = ptr[col0 + q];
      if (G.src[q] >= SRC_MASS && G.src[q] <= SRC_VZ) G.needv = 1;
      if (G.src[q] >= SRC_FX && G.src[q] <= SRC_FZ) G.needf = 1;
    }
    k_chunk_sums<<<maxtiles, kTile, 0, st>>>(e.d_vm(), e.d_force(), e.d_mask(), F.groupbit, c.idx_out.as<int>(),
                                             c.start.as<int>(), c.tileoff.as<int>(), nchunk, G, (long long)maxtiles,
                                             partial + (size_t)col0 * (size_t)maxtiles);
    T.launches++;
  }
  k_chunk_fold<<<div_up((long long)F.ncol * nchunk, 256), 256, 0, st>>>(partial, (long long)maxtiles, c.tileoff.as<int>(),
                                                                        nchunk, F.ncol, samplemask, acc);
  SF_HIP(hipGetLastError());
  T.launches++;
}

ChunkCompute& chunk_of(ChunkSet& T, const AveFix& F)
{
  ChunkCompute* c = T.find(F.S.chunk);
  if (!c) fail("Chunk/atom compute does not exist for fix ave/chunk");
  if (c->B.nchunk != F.nchunk) fail("fix ave/chunk %s: the chunk compute %s was redefined", F.S.id.c_str(), F.S.chunk.c_str());
  return *c;
}

// the centre of layer m of binned dimension a
double layer_centre(const ChunkBins& B, int a, int m) { return B.offset[a] + ((double)m + 0.5) * B.delta[a]; }

void chunk_coords(const ChunkBins& B, int chunk0, double* xyz)   // chunk0 = chunk ID - 1
{
  int rest = chunk0;
  for (int a = B.ndim - 1; a >= 0; a--) {
    xyz[a] = layer_centre(B, a, rest % B.nlayers[a]);
    rest /= B.nlayers[a];
  }
}

void write_output(AveFix& F, const ChunkBins& B)
{
  FILE* fp = F.file.fp();
  if (!fp) return;
  const int nv = (int)F.S.values.size();
  fail_if(F.file.begin_block());
  double total = 0.0;
  for (int c = 0; c < F.nchunk; c++) total += F.count[c];
  const std::string vfmt = " " + (F.S.format.empty() ? std::string("%g") : F.S.format);
  fprintf(fp, "%lld %d %g\n", F.out_step, F.nchunk, total);
  double xyz[3];
  for (int c = 0; c < F.nchunk; c++) {
    fprintf(fp, "  %d", c + 1);
    chunk_coords(B, c, xyz);
    for (int a = 0; a < B.ndim; a++) fprintf(fp, " %g", xyz[a]);
    fprintf(fp, " %g", F.count[c]);
    for (int j = 0; j < nv; j++) fprintf(fp, vfmt.c_str(), F.values[(size_t)c * nv + j]);
    fputc('\n', fp);
  }
  fail_if(F.file.end_block());
}

// the accumulator of Nrepeat samples -> Ncount and the value columns of one output (the rules of DESIGN.md section 14)
void make_output(SfLammps& L, AveFix& F, const ChunkBins& B)
{
  hipStream_t st = L.eng.stream();
  const int nchunk = F.nchunk, nv = (int)F.S.values.size();
  const size_t na = (size_t)F.ncol * (size_t)nchunk;
  F.h_acc.resize(na);
  SF_HIP(hipMemcpyAsync(F.h_acc.data(), F.acc.p, sizeof(double) * na, hipMemcpyDeviceToHost, st));
  SF_HIP(hipMemsetAsync(F.acc.p, 0, sizeof(double) * na, st));
  SF_HIP(hipStreamSynchronize(st));
  const double nrep = (double)F.S.nrepeat, V = B.volume;
  const bool all = F.S.norm == 0;
  std::vector<double> res((size_t)(1 + nv) * nchunk);   // per-output results, [1 + nvalues][nchunk]: Ncount, then the values
  if (F.S.running && F.run_acc.empty()) {
    F.run_acc.assign(na, 0.0);
    F.run_res.assign(res.size(), 0.0);
  }
  if (F.S.running)
    for (size_t k = 0; k < na; k++) F.run_acc[k] += F.h_acc[k];
  const std::vector<double>& A = F.S.running ? F.run_acc : F.h_acc;   // what norm all divides
  for (int c = 0; c < nchunk; c++) {
    res[c] = F.h_acc[c] / nrep;
    for (int j = 0; j < nv; j++) {
      const size_t at = (size_t)(j + 1) * nchunk + c;
      const int source = F.S.values[j].source;
      double r;
      if (!per_atom_value(source)) r = F.h_acc[at] / nrep / V;
      else if (all) r = A[c] > 0.0 ? A[at] / A[c] : 0.0;
      else r = F.h_acc[at] / nrep;
      res[at] = r;
    }
  }
  F.noutputs++;
  F.count.resize(nchunk);
  F.values.resize((size_t)nchunk * nv);
  if (F.S.running)
    for (size_t k = 0; k < res.size(); k++) F.run_res[k] += res[k];
  const double nout = (double)F.noutputs;
  for (int c = 0; c < nchunk; c++) {
    F.count[c] = F.S.running ? F.run_res[c] / nout : res[c];
    for (int j = 0; j < nv; j++) {
      const size_t at = (size_t)(j + 1) * nchunk + c;
      const bool mean = F.S.running && !(all && per_atom_value(F.S.values[j].source));
      F.values[(size_t)c * nv + j] = mean ? F.run_res[at] / nout : res[at];
    }
  }
  F.out_step = L.eng.nsteps();
  F.have = true;
  write_output(F, B);
}

void sample(SfLammps& L, ChunkSet& T, AveFix& F)
{
  refuse_decomposed(L, "fix ave/chunk");
  ChunkCompute& c = chunk_of(T, F);
  group(L, T, c);
  launch_sums(L, T, F, c, F.acc.as<double>());
  if (F.S.sampled(L.eng.nsteps())) make_output(L, F, c.B);
}

bool fix_exists(const SfLammps& L, const std::string& id)
{
  ChunkSet* T = set_of(L);
  return T && T->find_fix(id);
}

bool unfix(SfLammps& L, const std::string& id)
{
  ChunkSet* T = set_of(L);
  return T && ave_take(L, T->fixes, id);
}

// does a fix ave/chunk name this compute (as its chunk compute or as a c_ value)?
bool uses_compute(const SfLammps& L, const std::string& id)
{
  const ChunkSet* T = set_of(L);
  if (!T) return false;
  for (const auto& f : T->fixes) {
    if (f->S.chunk == id) return true;
    for (const AveValue& v : f->S.values)
      if (v.source == AS_COMPUTE && v.id == id) return true;
  }
  return false;
}

long long next_step(const SfLammps& L, long long step)
{
  const ChunkSet* T = set_of(L);
  return T ? ave_next(T->fixes, step) : -1;
}

}  // namespace

const AveFixKind& ave_chunk_kind()
{
  static const AveFixKind kind = {"fix ave/chunk", fix_exists, unfix, uses_compute, next_step};
  return kind;
}

// ---- the compute ----

void chunk_compute_define(SfLammps& L, const std::vector<std::string>& w)
{
  if (chunk_style_is_compute(w)) {   // (c_CID: the chunk ID is a compute's column; sf_pchunk.hip holds it, the functions below forward)
    pchunk_atom_define(L, w);
    return;
  }
  refuse_decomposed(L, "compute chunk/atom");
  auto c = std::make_unique<ChunkCompute>();
  c->id = w[1];
  c->groupbit = L.eng.group_bit(w[2]);
  double lo[3], hi[3];
  int per[3];
  L.eng.box(lo, hi, per);
  const std::string err = parse_chunk_atom(w, lo, hi, per, &c->B);
  if (!err.empty()) fail("%s", err.c_str());
  c->keybits = 1;
  while ((1ll << c->keybits) <= (long long)c->B.nchunk) c->keybits++;   // ceil(log2(nchunk + 1))
  ensure_set(L).computes.push_back(std::move(c));
}

bool chunk_compute_shape(const SfLammps& L, const std::string& id, ComputeShape* s)
{
  ChunkSet* T = set_of(L);
  if (!T || !T->find(id)) return pchunk_atom_shape(L, id, s);
  *s = ComputeShape();
  s->kind = CK_PERATOM;
  s->n = 1;
  s->chunk = true;
  return true;
}

void chunk_compute_remove(SfLammps& L, const std::string& id)
{
  if (ChunkSet* T = set_of(L)) compute_take(L, T->computes, id);   // (a frame queued on the stream may still read its buffer)
  pchunk_atom_remove(L, id);
}

const double* chunk_compute_values(SfLammps& L, const std::string& id)
{
  ChunkSet* T = set_of(L);
  ChunkCompute* c = T ? T->find(id) : nullptr;
  if (!c)
    if (const double* val = pchunk_atom_values(L, id)) return val;
  if (!c) fail("Could not find compute ID %s", id.c_str());
  if (!c->assigned.is_now(L.eng)) assign(L, *T, *c);
  else refuse_decomposed(L, "compute chunk/atom");
  return c->val.as<double>();
}

void chunk_invalidate(SfLammps& L)
{
  if (ChunkSet* T = set_of(L))
    for (auto& c : T->computes) {
      c->assigned.clear();
      c->grouped.clear();
    }
}

// ---- the fix ----

void ave_chunk_fix_command(SfLammps& L, const std::string& line)
{
  std::vector<std::string> w;
  const std::string qerr = split_quoted(line, &w);
  if (!qerr.empty()) fail("%s", qerr.c_str());
  auto F = std::make_unique<AveFix>();
  fail_if(parse_ave_chunk(w, &F->S));
  refuse_decomposed(L, "fix ave/chunk");
  F->groupbit = L.eng.group_bit(F->S.group);
  ChunkSet& T = ensure_set(L);
  if (ave_fix_exists(L, F->S.id))
    fail("fix ave/chunk %s: this fix ID is in use (unfix it first)", F->S.id.c_str());
  fail_if(check_ave_chunk_id(compute_shape(L, F->S.chunk)));
  ChunkCompute* c = T.find(F->S.chunk);
  if (!c)
    fail("fix ave/chunk: chunk/atom compute %s takes its chunk IDs from a compute (c_ID), which is not supported (the output "
         "needs layer coordinates and a fixed Nchunk; the per-chunk computes reduce over such chunks)", F->S.chunk.c_str());
  for (const AveValue& v : F->S.values)
    if (v.source == AS_COMPUTE) check_compute_value(L, v);
  F->nchunk = c->B.nchunk;
  F->ncol = 1 + (int)F->S.values.size();
  F->S.begin(L.eng.nsteps());
  hipStream_t st = L.eng.stream();
  const size_t na = sizeof(double) * (size_t)F->ncol * (size_t)F->nchunk;
  F->acc.get(na, st);
  SF_HIP(hipMemsetAsync(F->acc.p, 0, na, st));
  std::string titles[3] = {"# Chunk-averaged data for fix " + F->S.id + " and group " + F->S.group,
                           "# Timestep Number-of-chunks Total-count", "# Chunk"};
  for (int a = 0; a < c->B.ndim; a++) titles[2] += " Coord" + std::to_string(a + 1);
  titles[2] += " Ncount";
  for (const AveValue& v : F->S.values) titles[2] += " " + v.word;
  fail_if(F->file.open(F->S, "ave/chunk", F->S.id, titles, 3));
  T.fixes.push_back(std::move(F));
}

void ave_chunk_sample_due(SfLammps& L)
{
  ChunkSet* T = set_of(L);
  if (!T) return;
  const long long step = L.eng.nsteps();
  for (auto& f : T->fixes) {
    if (f->S.catch_up(step))   // (the samples of the output that was under way are dropped)
      SF_HIP(hipMemsetAsync(f->acc.p, 0, sizeof(double) * (size_t)f->ncol * (size_t)f->nchunk, L.eng.stream()));
    if (f->S.due(step)) sample(L, *T, *f);
  }
}

}  // namespace sf

using sf::handle;

extern "C" {

long long sf_lammps_ave_chunk(void* ptr, const char* id, long long max, long long* step, int* ndim, int* nvalues, double* coord,
                              double* count, double* values)
{
  long long n = 0;
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id) sf::fail("sf_lammps_ave_chunk: null argument");
  sf::ChunkSet* T = sf::set_of(L);
  sf::AveFix* F = T ? T->find_fix(id) : nullptr;
  if (!F) sf::fail("Could not find fix ave/chunk ID %s", id);
  if (!F->have) sf::fail("fix ave/chunk %s has made no output yet (the first one is due at a multiple of Nfreq)", id);
  const sf::ChunkBins& B = sf::chunk_of(*T, *F).B;
  const int nv = (int)F->S.values.size();
  if (step) *step = F->out_step;
  if (ndim) *ndim = B.ndim;
  if (nvalues) *nvalues = nv;
  n = F->nchunk;
  if (n <= max) {
    if (!coord || !count || !values) sf::fail("sf_lammps_ave_chunk: null argument");
    for (int c = 0; c < F->nchunk; c++) sf::chunk_coords(B, c, coord + (size_t)c * B.ndim);
    std::copy(F->count.begin(), F->count.end(), count);
    std::copy(F->values.begin(), F->values.end(), values);
  }
  SF_API_END(n)
}

long long sf_lammps_ave_chunk_names(void* ptr, const char* id, long long max, char* names)
{
  long long n = 0;
  SF_API_BEGIN
  if (!id) sf::fail("sf_lammps_ave_chunk_names: null argument");
  sf::ChunkSet* T = sf::set_of(*handle(ptr));
  sf::AveFix* F = T ? T->find_fix(id) : nullptr;
  if (!F) sf::fail("Could not find fix ave/chunk ID %s", id);
  std::string s;
  for (const sf::AveValue& v : F->S.values) s += (s.empty() ? "" : " ") + v.word;
  n = (long long)s.size() + 1;
  if (n <= max) {
    if (!names) sf::fail("sf_lammps_ave_chunk_names: null argument");
    std::memcpy(names, s.c_str(), (size_t)n);
  }
  SF_API_END(n)
}

int sf_lammps_ave_chunk_launches(void* ptr, long long* launches)
{
  SF_API_BEGIN
  if (!launches) sf::fail("sf_lammps_ave_chunk_launches: null argument");
  const sf::ChunkSet* T = sf::set_of(*handle(ptr));
  *launches = T ? T->launches : 0;
  SF_API_END(0)
}

int sf_lammps_ave_chunk_cost(void* ptr, const char* id, double* out3)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id || !out3) sf::fail("sf_lammps_ave_chunk_cost: null argument");
  sf::ChunkSet* T = sf::set_of(L);
  sf::AveFix* F = T ? T->find_fix(id) : nullptr;
  if (!F) sf::fail("Could not find fix ave/chunk ID %s", id);
  sf::refuse_decomposed(L, "fix ave/chunk");
  sf::ChunkCompute& c = sf::chunk_of(*T, *F);
  hipStream_t st = L.eng.stream();
  hipEvent_t ev[4];
  for (hipEvent_t& e : ev) SF_HIP(hipEventCreate(&e));
  struct EvGuard {
    hipEvent_t* ev;
    ~EvGuard()
    {
      for (int k = 0; k < 4; k++) (void)hipEventDestroy(ev[k]);
    }
  } guard{ev};
  // (the c_ columns are evaluated outside the time: they have a cost of their own, sf_lammps_compute_atom_cost)
  for (const sf::AveValue& v : F->S.values)
    if (v.source == sf::AS_COMPUTE) (void)sf::atom_compute_values(L, v.id, nullptr);
  const size_t na = sizeof(double) * (size_t)F->ncol * (size_t)F->nchunk;
  double* scratch = static_cast<double*>(F->cost_acc.get(na, st));   // (the sums go here: the fix's accumulator is untouched)
  SF_HIP(hipMemsetAsync(scratch, 0, na, st));
  SF_HIP(hipEventRecord(ev[0], st));
  sf::assign(L, *T, c);
  SF_HIP(hipEventRecord(ev[1], st));
  sf::group_sorted(L, *T, c);
  c.grouped.set(L.eng);
  SF_HIP(hipEventRecord(ev[2], st));
  sf::launch_sums(L, *T, *F, c, scratch);
  SF_HIP(hipEventRecord(ev[3], st));
  SF_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < 3; k++) {
    float ms = 0.f;
    SF_HIP(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
    out3[k] = (double)ms;
  }
  SF_API_END(0)
}

}  // extern "C"
