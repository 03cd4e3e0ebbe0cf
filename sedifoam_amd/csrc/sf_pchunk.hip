// sf_pchunk.hip -- chunks that a compute defines, and per-chunk sums ([3P] LAMMPS names and rules):
//   compute ID group chunk/atom c_CID | c_CID[k] [compress no|yes] [nchunk once|every] [ids every] [limit 0] [discard yes] [pbc no]
//       one column: raw = (int) of the named per-atom column for a grain of the group, 0 outside it; raw < 1 is chunk 0.
//       compress no: the chunk ID is raw, Nchunk the largest raw (nchunk once: of the first evaluation, kept; a larger raw is
//       then chunk 0).  compress yes: the distinct raw values in ascending order are chunks 1 .. Nchunk, the originals kept.
//   compute ID group property/chunk CID count [id]       grains per chunk, the original ID (compress yes)
//   compute ID group com/chunk CID                        sum m xu / sum m on the unwrapped positions, three columns
//   compute ID group vcm/chunk CID                        sum m v / sum m, three columns
//   compute ID group gyration/chunk CID [tensor]          sqrt(sum m |xu - xcm|^2 / sum m), or the six sums over sum m
//       global arrays of Nchunk rows; a grain counts when it is in the compute's group and has a chunk ID > 0.
// A value is evaluated from the state AT THE MOMENT OF THE OUTPUT and nothing is stored back into the run.
//
// One evaluation of the chunk/atom compute, on the engine's stream:
//   k_pca_assign     one lane per owned grain: the column value cast to the key (0: excluded), the atom index
//   radix sort       stable (key, index) pairs over 31 key bits (sf_sort.hip): the grains of a chunk stay in index order
//   k_pca_heads + scan   compress yes only: 1 at the first sorted position of every positive key, then its exclusive scan
//   k_pca_scatter    the dense chunk ID of every sorted position, the column scattered back by index, the list of originals,
//                    Nchunk -- which then reaches the host in ONE 4-byte copy, because the arrays need a shape
// One evaluation of a per-chunk compute (gyration: two, the second around the centres of the first):
//   k_pc_segscan     a wave takes 64 consecutive sorted grains, gathers their records through the index, forms up to six
//                    products in registers and runs a segmented inclusive scan keyed by chunk across its lanes.  The last lane
//                    of a segment that lies inside the wave and is neither its first nor its last segment stores the chunk's
//                    row; the first and the last segment go to two carry entries per wave
//   k_pc_segscan     again over the carry entries (64 of them per wave), and again, until one wave holds what is left and
//                    closes every segment: ceil(log32 n) launches whatever Nchunk is, never a block per chunk
//   k_pc_finish      one lane per (chunk, column): the division by sum m and gyration's root, operation by operation
// No floating-point atomics: which additions are made in which order follows from the sorted order alone, so the same
// state gives the same bits.  Nothing but Nchunk is copied to the host before a query.
#include <algorithm>
#include <climits>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_compute_atom.h"
#include "sf_compute_ids.h"
#include "sf_displace.h"
#include "sf_pchunk.h"
#include "sf_pchunk_parse.h"

namespace sf {
namespace {

constexpr int kPBlock = 256;   // four waves

// ---- the chunk/atom compute ----

__global__ __launch_bounds__(kPBlock) void k_pca_assign(const double* col, const int* mask, int n, int groupbit, int limit,
                                                        unsigned* key, int* idx)
{
  const int i = blockIdx.x * kPBlock + threadIdx.x;
  if (i >= n) return;
  int raw = 0;
  if (mask[i] & groupbit) {
    const double v = col[i];
    if (v >= 1.0 && v < 2147483648.0) raw = (int)v;   // (truncation toward zero; anything below 1 or not an int is chunk 0)
    if (raw > limit) raw = 0;
  }
  key[i] = (unsigned)raw;
  idx[i] = i;
}

__global__ __launch_bounds__(kPBlock) void k_pca_heads(const unsigned* key, int n, int* head)
{
  const int p = blockIdx.x * kPBlock + threadIdx.x;
  if (p >= n) return;
  const unsigned k = key[p];
  head[p] = (k > 0u && (p == 0 || key[p - 1] != k)) ? 1 : 0;
}

// sorted position p: its chunk ID to chunk[p] and, as a double, to the column of atom idx[p]; compress: the original of a
// chunk to ids[chunk - 1] by the head of its segment (ids has n entries: there are no more distinct values than grains).
// The lane of the last position stores Nchunk (compress no: the largest key)
__global__ __launch_bounds__(kPBlock) void k_pca_scatter(const unsigned* key, const int* idx, const int* head, const int* rank,
                                                         int n, int compress, double* val, int* chunk, int* ids, int* nchunk)
{
  const int p = blockIdx.x * kPBlock + threadIdx.x;
  if (p >= n) return;
  const int k = (int)key[p];
  int c = k;
  if (compress) {
    c = k > 0 ? rank[p] + head[p] : 0;
    if (head[p]) ids[c - 1] = k;
  }
  chunk[p] = c;
  val[idx[p]] = (double)c;
  if (p == n - 1) *nchunk = c;
}

// ---- the per-chunk sums ----

enum Mode { M_COUNT, M_VCM, M_COM, M_GYR };
// the columns of a sums row.  M_COUNT: count.  M_VCM: m, m vx, m vy, m vz.  M_COM: count, m, m xu, m yu, m zu.
// M_GYR: m dx dx, m dy dy, m dz dz, m dx dy, m dx dz, m dy dz around the centre of the M_COM row of the same chunk
__host__ __device__ constexpr int mode_cols(int mode) { return mode == M_COUNT ? 1 : (mode == M_VCM ? 4 : (mode == M_COM ? 5 : 6)); }

struct PSrc {
  const double4* xr;
  const double4* vm;
  const int* mask;
  const int* tag;
  const int* idx;      // sorted position -> atom index
  const int* chunk;    // sorted position -> chunk ID
  int groupbit;
  ImageView V;
  const double* com;   // M_GYR: the M_COM rows [nchunk][5]
  int nchunk;
};

// the centre of mass of a chunk from its M_COM row: the one place where it is formed (k_pc_finish stores it, the second pass of
// gyration/chunk subtracts it)
__device__ __forceinline__ double com_of(const double* row, int a)
{
#pragma clang fp contract(off)
  const double m = row[1];
  return m > 0.0 ? row[2 + a] / m : 0.0;
}

template <int MODE>
__device__ __forceinline__ void products(const PSrc& A, int p, int key, double (&v)[mode_cols(MODE)])
{
#pragma clang fp contract(off)
  constexpr int NC = mode_cols(MODE);
  const int i = A.idx[p];
  if (key <= 0 || key > A.nchunk || !(A.mask[i] & A.groupbit)) {
    for (int c = 0; c < NC; c++) v[c] = 0.0;
    return;
  }
  const double m = A.vm[i].w;
  if constexpr (MODE == M_COUNT) {
    v[0] = 1.0;
  } else if constexpr (MODE == M_VCM) {
    const double4 u = A.vm[i];
    v[0] = m;
    v[1] = m * u.x;
    v[2] = m * u.y;
    v[3] = m * u.z;
  } else {
    int im[3];
    double xu[3];
    image_of(A.V, A.tag[i], im);
    unmap(A.xr[i], im, A.V, xu);
    if constexpr (MODE == M_COM) {
      v[0] = 1.0;
      v[1] = m;
      for (int a = 0; a < 3; a++) v[2 + a] = m * xu[a];
    } else {
      const double* row = A.com + 5 * (size_t)(key - 1);
      double d[3];
      // (a chunk of one grain: the grain is its own centre, whatever m x / m rounds to)
      for (int a = 0; a < 3; a++) d[a] = row[0] == 1.0 ? 0.0 : xu[a] - com_of(row, a);
      v[0] = m * (d[0] * d[0]);
      v[1] = m * (d[1] * d[1]);
      v[2] = m * (d[2] * d[2]);
      v[3] = m * (d[0] * d[1]);
      v[4] = m * (d[0] * d[2]);
      v[5] = m * (d[1] * d[2]);
    }
  }
}

// One wave per 64 consecutive entries.  ATOMS: entry p is sorted grain p (key A.chunk[p], values its products); otherwise entry
// p is (in_key[p], in_val[p][NC]), the carries of the launch before.  Equal keys are consecutive in both.  final: one wave
// holds every entry and closes every segment; otherwise the wave's first and last segment go to out_key / out_val [2 wave],
// [2 wave + 1] (a wave of one segment: the sum and a zero under the same key, so that equal keys stay consecutive) and the
// segments between them, which no other wave sees a part of, to their rows.  rows: [nchunk][NC], zero before the first launch
template <int MODE, bool ATOMS>
__global__ __launch_bounds__(kPBlock) void k_pc_segscan(PSrc A, const int* in_key, const double* in_val, int count, int final,
                                                        double* rows, int nchunk, int* out_key, double* out_val)
{
#pragma clang fp contract(off)
  constexpr int NC = mode_cols(MODE);
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * kPBlock + threadIdx.x) >> 6;
  const long long base = wave * 64;
  if (base >= count) return;   // (the whole wave)
  const int last = (count - base < 64 ? (int)(count - base) : 64) - 1;
  const bool valid = lane <= last;
  int key = -1;   // (a lane past the end: a segment of its own that stores nothing)
  double v[NC];
  for (int c = 0; c < NC; c++) v[c] = 0.0;
  if (valid) {
    const int p = (int)(base + lane);
    if (ATOMS) {
      key = A.chunk[p];
      products<MODE>(A, p, key, v);
    } else {
      key = in_key[p];
      for (int c = 0; c < NC; c++) v[c] = in_val[(size_t)NC * p + c];
    }
  }
  for (int off = 1; off < 64; off <<= 1) {
    const int kt = __shfl_up(key, off, 64);
    const bool take = lane >= off && kt == key;
    for (int c = 0; c < NC; c++) {
      const double t = __shfl_up(v[c], off, 64);
      if (take) v[c] += t;
    }
  }
  const int knext = __shfl_down(key, 1, 64);
  const int kfirst = __shfl(key, 0, 64), klast = __shfl(key, last, 64);
  if (!valid || (lane < last && knext == key)) return;   // (not the last lane of a segment)
  if (final || (key != kfirst && key != klast)) {
    if (key > 0 && key <= nchunk)
      for (int c = 0; c < NC; c++) rows[(size_t)NC * (key - 1) + c] = v[c];
    return;
  }
  const size_t e = 2 * (size_t)wave + (key == kfirst ? 0 : 1);
  out_key[e] = key;
  for (int c = 0; c < NC; c++) out_val[NC * e + c] = v[c];
  if (kfirst == klast) {
    out_key[e + 1] = key;
    for (int c = 0; c < NC; c++) out_val[NC * (e + 1) + c] = 0.0;
  }
}

struct Props {
  int n;
  int p[8];
};

// out[m][j], one lane per entry.  rows: the sums of this compute's mode; com: the M_COM rows (gyration/chunk)
template <int MODE>
__global__ __launch_bounds__(kPBlock) void k_pc_finish(const double* rows, const double* com, const int* ids, Props P, int tensor,
                                                       int nchunk, int ncol, double* out)
{
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * kPBlock + threadIdx.x;
  if (t >= (long long)nchunk * ncol) return;
  const int m = (int)(t / ncol), j = (int)(t % ncol);
  double r = 0.0;
  if (MODE == M_COUNT) {
    r = P.p[j] == PP_COUNT ? rows[m] : (double)ids[m];
  } else if (MODE == M_VCM) {
    const double mass = rows[4 * (size_t)m];
    r = mass > 0.0 ? rows[4 * (size_t)m + 1 + j] / mass : 0.0;
  } else if (MODE == M_COM) {
    r = com_of(rows + 5 * (size_t)m, j);
  } else {
    const double mass = com[5 * (size_t)m + 1];
    const double* s = rows + 6 * (size_t)m;
    if (mass > 0.0) {
      if (tensor) r = s[j] / mass;
      else {
        const double sxy = s[0] + s[1];
        const double sum = sxy + s[2];
        r = sqrt_rn(sum / mass);
      }
    }
  }
  out[t] = r;
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

struct PChunkAtom {
  std::string id;
  int groupbit = 1;
  ChunkRefSpec S;
  int nchunk = 0;          // of the last evaluation
  bool have_nchunk = false;   // nchunk once: the first evaluation has fixed it
  DeviceScratch val, key_in, idx_in, key_out, idx_out, head, rank, chunk, ids, d_nchunk;
  RawTmp sort_tmp, scan_tmp;
  StateStamp made;
  long long launches = 0, host_copies = 0;   // of this compute and of the per-chunk computes over it
};

struct PChunkCompute {
  std::string id;
  int groupbit = 1;
  PChunkSpec S;
  DeviceScratch rows, rows2, carry_key[2], carry_val[2], out;
  int nrows = 0;   // of the last evaluation
  StateStamp made;
  std::string who() const { return std::string("compute ") + pchunk_style_name(S.style); }
};

struct PChunkSet {
  std::vector<std::unique_ptr<PChunkAtom>> atoms;
  std::vector<std::unique_ptr<PChunkCompute>> computes;
  PChunkAtom* find_atom(const std::string& id) const
  {
    for (auto& c : atoms)
      if (c->id == id) return c.get();
    return nullptr;
  }
  PChunkCompute* find(const std::string& id) const
  {
    for (auto& c : computes)
      if (c->id == id) return c.get();
    return nullptr;
  }
};

PChunkSet* set_of(const SfLammps& L) { return L.pchunks.get<PChunkSet>(); }
PChunkSet& ensure_set(SfLammps& L) { return L.pchunks.ensure<PChunkSet>(); }

// assign, sort, renumber, scatter; Nchunk to the host
void evaluate_atom(SfLammps& L, PChunkAtom& c)
{
  refuse_decomposed(L, "compute chunk/atom");
  // (the compute behind c_CID may have been removed and defined anew as something else)
  fail_if(check_chunk_atom_value(compute_shape(L, c.S.cid), c.S.index));
  if (c.made.is_now(L.eng)) return;
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int n = e.nlocal();
  int nc = 0;
  const double* col = atom_compute_values(L, c.S.cid, &nc);   // (once per step however many ask)
  if (c.S.index > nc) fail("Compute chunk/atom compute vector is accessed out-of-range");
  col += (size_t)(c.S.index > 0 ? c.S.index - 1 : 0) * (size_t)n;
  const size_t m = (size_t)std::max(n, 1);
  double* val = static_cast<double*>(c.val.get(sizeof(double) * m, st));
  unsigned* key_in = static_cast<unsigned*>(c.key_in.get(sizeof(unsigned) * m, st));
  int* idx_in = static_cast<int*>(c.idx_in.get(sizeof(int) * m, st));
  unsigned* key_out = static_cast<unsigned*>(c.key_out.get(sizeof(unsigned) * m, st));
  int* idx_out = static_cast<int*>(c.idx_out.get(sizeof(int) * m, st));
  int* chunk = static_cast<int*>(c.chunk.get(sizeof(int) * m, st));
  int* ids = static_cast<int*>(c.ids.get(sizeof(int) * m, st));
  int* d_nchunk = static_cast<int*>(c.d_nchunk.get(sizeof(int), st));
  int* head = nullptr;
  int* rank = nullptr;
  if (c.S.compress) {
    head = static_cast<int*>(c.head.get(sizeof(int) * m, st));
    rank = static_cast<int*>(c.rank.get(sizeof(int) * m, st));
  }
  int found = 0;
  if (n > 0) {
    const int nb = div_up(n, kPBlock);
    const int limit = c.S.rows_fixed() && c.have_nchunk ? c.nchunk : INT_MAX;
    k_pca_assign<<<nb, kPBlock, 0, st>>>(col, e.d_mask(), n, c.groupbit, limit, key_in, idx_in);
    SF_HIP(hipGetLastError());
    sort_pairs_u32(c.sort_tmp.p, c.sort_tmp.n, key_in, key_out, idx_in, idx_out, n, 31, st);
    c.launches += 2;   // (the sort counts as one)
    if (c.S.compress) {
      k_pca_heads<<<nb, kPBlock, 0, st>>>(key_out, n, head);
      SF_HIP(hipGetLastError());
      exclusive_scan_i32(c.scan_tmp.p, c.scan_tmp.n, head, rank, n, st);
      c.launches += 2;   // (and so does the scan)
    }
    k_pca_scatter<<<nb, kPBlock, 0, st>>>(key_out, idx_out, head, rank, n, c.S.compress ? 1 : 0, val, chunk, ids, d_nchunk);
    SF_HIP(hipGetLastError());
    c.launches++;
    SF_HIP(hipMemcpyAsync(&found, d_nchunk, sizeof(int), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    c.host_copies++;
  }
  if (!(c.S.rows_fixed() && c.have_nchunk)) c.nchunk = found;
  c.have_nchunk = true;
  c.made.set(e);
}

PChunkAtom& atom_of(const SfLammps& L, const PChunkCompute& c)
{
  PChunkSet* T = set_of(L);
  PChunkAtom* a = T ? T->find_atom(c.S.chunk) : nullptr;
  if (!a) fail("Chunk/atom compute does not exist for %s", c.who().c_str());
  return *a;
}

// the segmented sums of one mode over the grouping of `a`, into rows[nchunk][NC]
template <int MODE>
void launch_sums(SfLammps& L, PChunkAtom& a, PChunkCompute& c, const PSrc& A, double* rows)
{
  constexpr int NC = mode_cols(MODE);
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int n = e.nlocal(), nchunk = a.nchunk;
  if (nchunk > 0) SF_HIP(hipMemsetAsync(rows, 0, sizeof(double) * (size_t)NC * (size_t)nchunk, st));
  if (n <= 0 || nchunk <= 0) return;
  int count = n, nw = div_up(count, 64);
  // the carries of level k: two per wave; the two buffers alternate
  const size_t cap0 = 2 * (size_t)nw, cap1 = 2 * (size_t)div_up((long long)cap0, 64);
  int* ckey[2] = {static_cast<int*>(c.carry_key[0].get(sizeof(int) * cap0, st)),
                  static_cast<int*>(c.carry_key[1].get(sizeof(int) * cap1, st))};
  double* cval[2] = {static_cast<double*>(c.carry_val[0].get(sizeof(double) * NC * cap0, st)),
                     static_cast<double*>(c.carry_val[1].get(sizeof(double) * NC * cap1, st))};
  bool final = count <= 64;
  k_pc_segscan<MODE, true><<<div_up(nw, kPBlock / 64), kPBlock, 0, st>>>(A, nullptr, nullptr, count, final ? 1 : 0, rows, nchunk,
                                                                          ckey[0], cval[0]);
  SF_HIP(hipGetLastError());
  a.launches++;
  for (int src = 0; !final; src ^= 1) {
    count = 2 * nw;
    nw = div_up(count, 64);
    final = count <= 64;
    k_pc_segscan<MODE, false><<<div_up(nw, kPBlock / 64), kPBlock, 0, st>>>(A, ckey[src], cval[src], count, final ? 1 : 0, rows,
                                                                             nchunk, ckey[src ^ 1], cval[src ^ 1]);
    SF_HIP(hipGetLastError());
    a.launches++;
  }
}

template <int MODE>
void launch_finish(SfLammps& L, PChunkAtom& a, PChunkCompute& c, const double* rows, const double* com, double* out)
{
  const long long cells = (long long)a.nchunk * c.S.ncols();
  if (cells <= 0) return;
  Props P{};
  P.n = (int)c.S.props.size();
  for (int k = 0; k < P.n; k++) P.p[k] = c.S.props[k];
  k_pc_finish<MODE><<<div_up(cells, kPBlock), kPBlock, 0, L.eng.stream()>>>(rows, com, a.ids.as<int>(), P, c.S.tensor ? 1 : 0,
                                                                           a.nchunk, c.S.ncols(), out);
  SF_HIP(hipGetLastError());
  a.launches++;
}

// what a per-chunk compute needs of the engine and of its chunk/atom compute as they are now (checked at the compute line and
// at every evaluation)
PChunkAtom& check_compute(SfLammps& L, PChunkCompute& c)
{
  refuse_decomposed(L, c.who().c_str());
  const ComputeShape shape = compute_shape(L, c.S.chunk);
  PChunkSet* T = set_of(L);
  PChunkAtom* a = T ? T->find_atom(c.S.chunk) : nullptr;
  fail_if(check_pchunk_chunk(c.S, shape, a != nullptr, a && a->S.compress));
  return *a;
}

void evaluate(SfLammps& L, PChunkCompute& c)
{
  PChunkAtom& a = check_compute(L, c);
  evaluate_atom(L, a);
  if (c.made.is_now(L.eng)) return;
  DemEngine& e = L.eng;
  hipStream_t st = e.stream();
  const int nchunk = a.nchunk, style = c.S.style;
  const size_t nr = (size_t)std::max(nchunk, 1);
  PSrc A{e.d_xr(), e.d_vm(), e.d_mask(), e.d_tag(), a.idx_out.as<int>(), a.chunk.as<int>(), c.groupbit, ImageView{}, nullptr, nchunk};
  if (style == PC_COM || style == PC_GYRATION) A.V = image_view(L, c.who().c_str());
  double* out = static_cast<double*>(c.out.get(sizeof(double) * nr * (size_t)c.S.ncols(), st));
  if (style == PC_PROPERTY) {
    if (c.S.props.size() > 8) fail("compute property/chunk: at most 8 values");
    double* rows = static_cast<double*>(c.rows.get(sizeof(double) * nr * mode_cols(M_COUNT), st));
    launch_sums<M_COUNT>(L, a, c, A, rows);
    launch_finish<M_COUNT>(L, a, c, rows, nullptr, out);
  } else if (style == PC_VCM) {
    double* rows = static_cast<double*>(c.rows.get(sizeof(double) * nr * mode_cols(M_VCM), st));
    launch_sums<M_VCM>(L, a, c, A, rows);
    launch_finish<M_VCM>(L, a, c, rows, nullptr, out);
  } else {
    double* rows = static_cast<double*>(c.rows.get(sizeof(double) * nr * mode_cols(M_COM), st));
    launch_sums<M_COM>(L, a, c, A, rows);
    if (style == PC_COM) {
      launch_finish<M_COM>(L, a, c, rows, nullptr, out);
    } else {   // (the second pass, around the centres of the first)
      double* rows2 = static_cast<double*>(c.rows2.get(sizeof(double) * nr * mode_cols(M_GYR), st));
      A.com = rows;
      launch_sums<M_GYR>(L, a, c, A, rows2);
      launch_finish<M_GYR>(L, a, c, rows2, rows, out);
    }
  }
  c.nrows = nchunk;
  c.made.set(e);
}

// ---- the kind (sf_compute_ids.h) ----

bool is_style(const std::string& style) { return pchunk_style_of(style) >= 0; }

void define(SfLammps& L, const std::vector<std::string>& w)
{
  auto c = std::make_unique<PChunkCompute>();
  c->id = w[1];
  c->groupbit = L.eng.group_bit(w[2]);
  fail_if(parse_pchunk(w, &c->S));
  check_compute(L, *c);
  // (refused where image counts cannot be kept; makes the table)
  if (c->S.style == PC_COM || c->S.style == PC_GYRATION) (void)image_view(L, c->who().c_str());
  ensure_set(L).computes.push_back(std::move(c));
}

bool shape(const SfLammps& L, const std::string& id, ComputeShape* s)
{
  PChunkSet* T = set_of(L);
  const PChunkCompute* c = T ? T->find(id) : nullptr;
  if (!c) return false;
  const PChunkAtom* a = T->find_atom(c->S.chunk);
  *s = ComputeShape();
  s->kind = CK_ARRAY;
  s->n = c->S.ncols();
  s->rows = a ? a->nchunk : 0;
  s->rows_vary = !a || !a->S.rows_fixed();
  return true;
}

void remove(SfLammps& L, const std::string& id)
{
  if (PChunkSet* T = set_of(L)) compute_take(L, T->computes, id);   // (a launch queued on the stream may still write its values)
}

void invalidate(SfLammps& L)
{
  if (PChunkSet* T = set_of(L)) {
    for (auto& c : T->atoms) c->made.clear();
    for (auto& c : T->computes) c->made.clear();
  }
}

}  // namespace

const ComputeKindOps& pchunk_compute_kind()
{
  static const ComputeKindOps kind = {is_style, define, remove, shape, invalidate};
  return kind;
}

// ---- the chunk/atom compute ----

void pchunk_atom_define(SfLammps& L, const std::vector<std::string>& w)
{
  refuse_decomposed(L, "compute chunk/atom");
  auto c = std::make_unique<PChunkAtom>();
  c->id = w[1];
  c->groupbit = L.eng.group_bit(w[2]);
  fail_if(parse_chunk_atom_compute(w, &c->S));
  fail_if(check_chunk_atom_value(compute_shape(L, c->S.cid), c->S.index));
  ensure_set(L).atoms.push_back(std::move(c));
}

bool pchunk_atom_shape(const SfLammps& L, const std::string& id, ComputeShape* s)
{
  PChunkSet* T = set_of(L);
  if (!T || !T->find_atom(id)) return false;
  *s = ComputeShape();
  s->kind = CK_PERATOM;
  s->n = 1;
  s->chunk = true;
  return true;
}

void pchunk_atom_remove(SfLammps& L, const std::string& id)
{
  if (PChunkSet* T = set_of(L)) compute_take(L, T->atoms, id);   // (a frame queued on the stream may still read its buffer)
}

const double* pchunk_atom_values(SfLammps& L, const std::string& id)
{
  PChunkSet* T = set_of(L);
  PChunkAtom* c = T ? T->find_atom(id) : nullptr;
  if (!c) return nullptr;
  evaluate_atom(L, *c);
  return c->val.as<double>();
}

// ---- the per-chunk computes ----

bool pchunk_holds(const SfLammps& L, const std::string& id)
{
  const PChunkSet* T = set_of(L);
  return T && T->find(id);
}

void pchunk_prepare(SfLammps& L, const std::string& id)
{
  PChunkSet* T = set_of(L);
  PChunkCompute* c = T ? T->find(id) : nullptr;
  if (!c) return;
  PChunkAtom& a = check_compute(L, *c);
  if (a.S.rows_fixed() && !a.have_nchunk) evaluate_atom(L, a);   // (nchunk once: the first evaluation fixes the rows)
}

const double* pchunk_array_device(SfLammps& L, const std::string& id, int* rows, int* ncols)
{
  PChunkSet* T = set_of(L);
  PChunkCompute* c = T ? T->find(id) : nullptr;
  if (!c) fail("Could not find compute ID %s", id.c_str());
  evaluate(L, *c);
  if (rows) *rows = c->nrows;
  if (ncols) *ncols = c->S.ncols();
  return c->out.as<double>();
}

const char* pchunk_uses_compute(const SfLammps& L, const std::string& id)
{
  const PChunkSet* T = set_of(L);
  if (!T) return nullptr;
  for (const auto& c : T->computes)
    if (c->S.chunk == id) {
      static const char* const who[kNumPChunkStyles] = {"compute property/chunk", "compute com/chunk", "compute vcm/chunk",
                                                        "compute gyration/chunk"};
      return who[c->S.style];
    }
  for (const auto& a : T->atoms)
    if (a->S.cid == id) return "compute chunk/atom";
  return nullptr;
}

}  // namespace sf

using sf::handle;

extern "C" {

// Nchunk of chunk/atom compute `id` (over c_CID) on the state as it stands; with Nchunk <= max, ids[Nchunk]: the original IDs
// under compress yes, 1 .. Nchunk otherwise.  launches / host_copies: made by the evaluations of this compute and of the
// per-chunk computes over it so far (the copies of the getters themselves are not among them)
long long sf_lammps_chunk_info(void* ptr, const char* id, long long max, int* ids, long long* launches, long long* host_copies)
{
  long long n = 0;
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id) sf::fail("sf_lammps_chunk_info: null argument");
  sf::PChunkSet* T = sf::set_of(L);
  sf::PChunkAtom* c = T ? T->find_atom(id) : nullptr;
  if (!c) sf::fail("Could not find a compute chunk/atom over c_ID with the ID %s", id);
  sf::evaluate_atom(L, *c);
  n = c->nchunk;
  if (launches) *launches = c->launches;
  if (host_copies) *host_copies = c->host_copies;
  if (n > 0 && n <= max) {
    if (!ids) sf::fail("sf_lammps_chunk_info: null argument");
    if (c->S.compress) {
      hipStream_t st = L.eng.stream();
      SF_HIP(hipMemcpyAsync(ids, c->ids.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
      SF_HIP(hipStreamSynchronize(st));
    } else {
      for (long long k = 0; k < n; k++) ids[k] = (int)(k + 1);
    }
  }
  SF_API_END(n)
}

// measurement (tools/pchunk_cost.py): GPU ms from HIP events of one evaluation now of chunk/atom compute `id` (over c_CID) and
// of every per-chunk compute over it -- the sort, the renumbering, the wait for the 4 bytes of Nchunk, the segmented sums and
// the finish; the compute behind c_CID is evaluated before the clock starts
int sf_lammps_chunk_cost(void* ptr, const char* id, double* ms)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!id || !ms) sf::fail("sf_lammps_chunk_cost: null argument");
  sf::PChunkSet* T = sf::set_of(L);
  sf::PChunkAtom* c = T ? T->find_atom(id) : nullptr;
  if (!c) sf::fail("Could not find a compute chunk/atom over c_ID with the ID %s", id);
  sf::refuse_decomposed(L, "compute chunk/atom");
  (void)sf::atom_compute_values(L, c->S.cid, nullptr);
  c->made.clear();
  for (auto& pc : T->computes)
    if (pc->S.chunk == c->id) pc->made.clear();
  *ms = sf::stream_ms(L.eng.stream(), [&] {
    sf::evaluate_atom(L, *c);
    for (auto& pc : T->computes)
      if (pc->S.chunk == c->id) sf::evaluate(L, *pc);
  });
  SF_API_END(0)
}

}  // extern "C"
