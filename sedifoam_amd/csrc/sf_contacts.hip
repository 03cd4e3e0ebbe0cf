// sf_contacts.hip -- `compute ID group pair/local v...` (the reference's name for it: `compute ID group gran/local ...`,
// cases/example-cases/BL24-TH1/in.lammps:33), `uncompute ID`, and the rows behind `dump ID group local ...` (sf_dump.hip) and
// sf_lammps_get_contacts: the contact network -- which pairs touch, and with what normal and tangential force.
//
// Not a port of the reference's compute_gran_local.cpp (PairGranHertzFixHistory::single() reads uninitialised values,
// docs/history_r01_r03.md section 6.5).  The semantics are those of [3P] compute pair/local, which calls Pair::single() at
// output time: a row is evaluated from the state at the moment of the output -- the x, v, omega a `dump custom` frame
// shows, the shear history sf_dem_get_history returns -- with shearupdate = false, and nothing is stored.
//   row     one touching pair (rsq < (radi + radj)^2), both atoms in the compute's group, written once: tag1 < tag2,
//           del = x(tag1) - x(tag2) by minimum image, forces on tag1
//   dist = r, eng = 0 (granular single() returns 0), force = r ccel (signed normal force, repulsive > 0),
//   fx fy fz = del ccel (the normal part), p1 p2 p3 = fs (the tangential force on tag1), p4 = |fs|
//   meff as the sub-step kernel takes it, the `fix freeze` override included.  Walls, fix cohesive and lubrication are not
//   in a row.
// The total pair force F comes from gran_history_law of sf_physics.h, unchanged; contact_ccel below restates the two
// normal-force lines of each law and fs = F - del ccel.  That subtraction costs p1..p3 a few ulp of the NORMAL force, not
// of themselves.
//
// Three launches on the engine's stream, all one lane per owned atom:
//   k_contact_count  the atom's partners with a higher tag, in the group, touching -> cnt[n + 1] (last element zero)
//   exclusive scan   its last element is the row count (one host read)
//   k_contact_rows   the atom's rows into [off[i], off[i + 1]), partners in ascending tag order, field-major columns
// and for text k_contact_lines, one lane per row, into the slots of the dump pipeline (sf_dump.hip).
// Order: atom index, then partner tag.  No atomics, no floating-point reduction: the same run gives the same rows in the
// same order with the same bits.
#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_compute_ids.h"
#include "sf_contacts.h"
#include "sf_dem_dispatch.h"
#include "sf_dump_fmt.h"

namespace sf {
namespace {

__device__ __forceinline__ Vec3 cv3(const double4& a) { return {a.x, a.y, a.z}; }

// the scalar both laws multiply del with: the two normal-force lines of hooke_history_law / hertz_history_law
// (sf_physics.h), restated; everything else of a row comes from the law itself
template <int STYLE>
__device__ __forceinline__ double contact_ccel(const GranParams& p, const ContactIn& c)
{
  const double rsqinv = c.rinv * c.rinv;
  const double vnnr = dot(c.vr, c.del);
  if (STYLE == 2) {
    const double polyhertz = sf_sqrt(c.reff);
    const double sqsn = sf_sqrt(p.h_sn * polyhertz * c.meff);
    const double damp = p.h_c56beta * vnnr * rsqinv;
    return polyhertz * p.h_cn * c.overlap * c.rinv - sqsn * damp;
  }
  const double damp = c.meff * p.gamman * vnnr * rsqinv;
  return p.kn * c.overlap * c.rinv - damp;
}

// slot s of atom i as k_thermo_virial (sf_thermo.hip) walks it: the neighbour's record -- the root's, moved to the image the
// word names, or the plain index -- and whether the pair is a row of atom i: a higher tag, in the group, touching
struct ContactSlot {
  int jraw, j, tagj;
  double4 xj;
  Vec3 del;
  double rsq;
};
__device__ __forceinline__ bool contact_slot(const DemPtrs& P, const StepParams& S, const int* tag, int groupbit, int i,
                                             const double4& xi4, int tagi, int s, ContactSlot& o)
{
  o.jraw = P.neigh[(size_t)s * (size_t)S.cap + i];
  o.j = neigh_index(o.jraw, S.roots);
  o.tagj = tag[o.j];
  if (o.tagj <= tagi || !(P.mask[o.j] & groupbit)) return false;
  o.xj = P.xr_in[o.j];
  if (S.roots && (o.jraw & kOwnBit)) shift_to_image(o.xj, o.jraw, S.prd);
  o.del = cv3(xi4) - cv3(o.xj);
  o.rsq = dot(o.del, o.del);
  const double radsum = xi4.w + o.xj.w;
  return o.rsq < radsum * radsum;
}

// cnt has n + 1 elements; lane n writes the zero the exclusive scan turns into the total
__global__ __launch_bounds__(256) void k_contact_count(DemPtrs P, StepParams S, const int* tag, int groupbit, int* cnt)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > S.nlocal) return;
  int c = 0;
  if (i < S.nlocal && (P.mask[i] & groupbit)) {
    const double4 xi4 = P.xr_in[i];
    const int tagi = tag[i], nn = P.numneigh[i];
    ContactSlot o;
    for (int s = 0; s < nn; s++) c += contact_slot(P, S, tag, groupbit, i, xi4, tagi, s, o) ? 1 : 0;
  }
  cnt[i] = c;
}

struct ContactOutCols {
  int *tag1, *tag2;   // [nrows]
  double* val;        // [kContactDoubles][nrows]
  int nrows;
};

// Lane i fills [off[i], off[i + 1]): the partners by repeated minimum over (tag, slot) -- a row of the list has a handful
// of them (k_rst_contacts, sf_restart.hip) -- so that neighbouring lanes store to neighbouring stretches of every column.
// The history of a pair is read where the force evaluation reads it: the own slot where this side's word carries
// kOwnBit, the owner's slot negated where it does not (the owner of a pair of two atoms of this GPU is the lower INDEX,
// which after a re-sort need not be the lower tag), zero without the touch bit.
template <int STYLE>
__global__ __launch_bounds__(256) void k_contact_rows(DemPtrs P, StepParams S, const int* tag, int groupbit, const int* off,
                                                      ContactOutCols C)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.nlocal) return;
  const int first = off[i], count = off[i + 1] - first;
  if (count <= 0) return;
  const size_t cap = (size_t)S.cap;
  const double4 xi4 = P.xr_in[i], vi4 = P.vm_in[i], wi4 = P.om_in[i];
  const Vec3 vi = cv3(vi4), wi = cv3(wi4);
  const double radi = xi4.w, mi = vi4.w;
  const int tagi = tag[i], nn = P.numneigh[i];
  ContactSlot o;
  // which of the first 64 slots are rows (the geometry is then not evaluated again per pick; later slots are tested anew)
  unsigned long long rowmask = 0ull;
  for (int s = 0; s < nn && s < 64; s++)
    if (contact_slot(P, S, tag, groupbit, i, xi4, tagi, s, o)) rowmask |= 1ull << s;
  long long prev = -1;
  for (int k = 0; k < count; k++) {
    long long best = 0x7fffffffffffffffll;
    for (int s = 0; s < nn; s++) {
      if (s < 64) {
        if (!((rowmask >> s) & 1ull)) continue;
        const int w = P.neigh[(size_t)s * cap + i];
        const long long key = ((long long)tag[neigh_index(w, S.roots)] << 32) | (long long)s;
        if (key > prev && key < best) best = key;
      } else if (contact_slot(P, S, tag, groupbit, i, xi4, tagi, s, o)) {
        const long long key = ((long long)o.tagj << 32) | (long long)s;
        if (key > prev && key < best) best = key;
      }
    }
    const int e = first + k;
    if (best == 0x7fffffffffffffffll || e >= C.nrows) return;   // (cannot happen: the count walked the same slots)
    prev = best;
    const int s = (int)(best & 0xffffffffll);
    contact_slot(P, S, tag, groupbit, i, xi4, tagi, s, o);
    const int jraw = o.jraw, j = o.j;
    const bool own = (jraw & kOwnBit) != 0;
    const double4 vj4 = P.vm_in[j], wj4 = P.om_in[j];
    const double radj = o.xj.w, mj = vj4.w;
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
    c.del = o.del;
    c.rsq = o.rsq;
    sf_sqrt_rsqrt(o.rsq, c.r, c.rinv);
    c.vr = vi - cv3(vj4);
    c.wsum = {radi * wi.x + radj * wj4.x, radi * wi.y + radj * wj4.y, radi * wi.z + radj * wj4.z};
    const PairScales m = pair_scales(mi, mj, radi, radj, c.r);
    c.overlap = m.overlap;
    c.meff = m.meff;
    c.reff = m.reff;
    if (S.freeze_bit) {   // pair_gran_hertzFix_history.cpp:188-189
      if (wi4.w != 0.0) c.meff = mj;
      if (wj4.w != 0.0) c.meff = mi;
    }
    ContactOut out;
    gran_history_law<STYLE>(S.gran, S.dt, false, c, sh, out);
    const double ccel = contact_ccel<STYLE>(S.gran, c);
    const Vec3 fn = {c.del.x * ccel, c.del.y * ccel, c.del.z * ccel};
    const Vec3 fs = out.F - fn;
    const size_t N = (size_t)C.nrows;
    C.tag1[e] = tagi;
    C.tag2[e] = o.tagj;
    C.val[CV_DIST * N + e] = c.r;
    C.val[CV_FORCE * N + e] = c.r * ccel;
    C.val[CV_FX * N + e] = fn.x;
    C.val[CV_FY * N + e] = fn.y;
    C.val[CV_FZ * N + e] = fn.z;
    C.val[CV_P1 * N + e] = fs.x;
    C.val[CV_P2 * N + e] = fs.y;
    C.val[CV_P3 * N + e] = fs.z;
    C.val[CV_P4 * N + e] = sqrt(dot(fs, fs));
  }
}

// one lane per row: `index` (the row number, 1-based) and the tags as "%d ", everything else as "%g ", then "\n" -- what
// k_dump_lines (sf_dump.hip) does per atom.  (The tags deliberately not as LAMMPS prints compute columns, "%g": that is
// the same bytes below 10^6 and corrupts a tag above, INTEGRATION.md.)
__global__ __launch_bounds__(256) void k_contact_lines(const int* tag1, const int* tag2, const double* val, long long nrows,
                                                       ContactCols cols, int stride, char* slots,
                                                       unsigned long long* len)
{
  const long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  char* p0 = slots + r * (long long)stride;
  char* p = p0;
  for (int k = 0; k < cols.n; k++) {
    const int c = cols.c[k];
    if (c == kContactIndex) p += fmt::format_d((int)(r + 1), p);
    else if (c == CV_TAG1) p += fmt::format_d(tag1[r], p);
    else if (c == CV_TAG2) p += fmt::format_d(tag2[r], p);
    else if (c == CV_ENG) p += fmt::format_g(0.0, p);
    else p += fmt::format_g(val[(size_t)c * (size_t)nrows + (size_t)r], p);
    *p++ = ' ';
  }
  *p++ = '\n';
  len[r] = (unsigned long long)(p - p0);
}

// ---- host side ----

const char* const kValueName[CV_COUNT] = {"dist", "force", "fx", "fy", "fz", "p1", "p2", "p3", "p4", "eng", "tag1", "tag2"};

struct Compute {
  std::string id;
  int groupbit = 1;
  std::vector<unsigned char> values;
};

struct ContactSet {
  std::vector<Compute> computes;
  DeviceScratch cnt, off, tags, vals;   // (a frame comes every N steps: no allocation per frame)
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  int* h_total = nullptr;   // pinned
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  long long launches = 0;
  ~ContactSet()
  {
    if (scan_tmp) (void)hipFree(scan_tmp);
    if (h_total) (void)hipHostFree(h_total);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  Compute* find(const std::string& id)
  {
    for (Compute& c : computes)
      if (c.id == id) return &c;
    return nullptr;
  }
};

ContactSet* set_of(const SfLammps& L) { return L.computes.get<ContactSet>(); }
ContactSet& ensure_set(SfLammps& L) { return L.computes.ensure<ContactSet>(); }

// what an evaluation needs of the engine as it is now (the compute command checks it, and every evaluation again: the
// pair style and the fixes may have changed since)
void refuse_unsupported(const SfLammps& L, const char* who)
{
  const DemEngine& e = L.eng;
  if (e.pair_lubricate_on())   // [3P] ComputePairLocal::init: a style without single()
    fail("%s: Pair style does not support compute pair/local (lubricate/poly has no single())", who);
  if (e.pair_gran_style() == 0)
    fail("%s: No pair style is defined for compute pair/local (a granular pair style is needed)", who);
  if (e.rigid_on())
    fail("%s: not while fix rigid/nve exists (the pair law then takes the masses of the bodies)", who);
  refuse_decomposed(L, who);
}

}  // namespace

bool DemEngine::contact_view(DemPtrs* P, StepParams* S) const
{
  *P = ptrs(cur_);
  *S = step_params(2, 0);
  return have_list_;
}

// ---- the kind (sf_compute_ids.h) ----
namespace {
bool is_style(const std::string& style) { return style == "pair/local" || style == "gran/local"; }

// compute ID group-ID pair/local v1 v2 ...  |  compute ID group-ID gran/local ...
void define(SfLammps& L, const std::vector<std::string>& w)
{
  Compute c;
  c.id = w[1];
  c.groupbit = L.eng.group_bit(w[2]);
  if (w.size() < 5) fail("Illegal compute pair/local command");
  refuse_unsupported(L, "compute pair/local");
  for (size_t k = 4; k < w.size(); k++) {
    int v = -1;
    for (int q = 0; q < CV_COUNT; q++)
      if (w[k] == kValueName[q]) v = q;
    if (v < 0 && w[k].size() >= 2 && w[k][0] == 'p' && std::isdigit((unsigned char)w[k][1])) {
      // [3P] ComputePairLocal: pN beyond what the pair style's single() provides (four values here)
      fail("Pair style does not have extra field requested by compute pair/local: %s (p1 .. p4 exist)", w[k].c_str());
    }
    if (v < 0) fail("Invalid keyword in compute pair/local command: %s", w[k].c_str());
    if ((int)c.values.size() >= kContactMaxCols) fail("Illegal compute pair/local command");
    c.values.push_back((unsigned char)v);
  }
  ensure_set(L).computes.push_back(std::move(c));
}

// (no wait for the stream, unlike the other kinds: a compute pair/local holds no device buffer of its own -- the rows are
// the set's scratch, which stays)
void remove(SfLammps& L, const std::string& id)
{
  ContactSet* S = set_of(L);
  if (Compute* c = S ? S->find(id) : nullptr) S->computes.erase(S->computes.begin() + (c - S->computes.data()));
}

bool shape(const SfLammps& L, const std::string& id, ComputeShape* s)
{
  ContactSet* S = set_of(L);
  const Compute* c = S ? S->find(id) : nullptr;
  if (!c) return false;
  *s = ComputeShape();
  s->kind = CK_LOCAL;
  s->n = (int)c->values.size();
  return true;
}

void invalidate(SfLammps&) {}   // (the rows are made anew at every request)
}  // namespace

const ComputeKindOps& pair_local_kind()
{
  static const ComputeKindOps kind = {is_style, define, remove, shape, invalidate};
  return kind;
}

void compute_lookup(const SfLammps& L, const std::string& id, std::vector<unsigned char>* values, int* groupbit)
{
  ContactSet* S = set_of(L);
  const Compute* c = S ? S->find(id) : nullptr;
  if (!c) fail("Could not find dump local compute ID %s", id.c_str());
  if (values) *values = c->values;
  if (groupbit) *groupbit = c->groupbit;
}

ContactRows contact_rows(SfLammps& L, int groupbit, double* ms)
{
  refuse_unsupported(L, "compute pair/local");
  ContactSet& T = ensure_set(L);
  DemEngine& e = L.eng;
  ContactRows R;
  const int n = e.nlocal();
  if (ms) *ms = 0.0;
  if (n <= 0) return R;
  DemPtrs P;
  StepParams S;
  if (!e.contact_view(&P, &S))
    fail("compute pair/local: no neighbour list yet (the contacts are those of the last force evaluation: run 0 first)");
  hipStream_t st = e.stream();
  if (!T.h_total) SF_HIP(hipHostMalloc(reinterpret_cast<void**>(&T.h_total), sizeof(int)));
  if (ms)
    for (hipEvent_t& ev : T.ev)
      if (!ev) SF_HIP(hipEventCreate(&ev));
  int* cnt = static_cast<int*>(T.cnt.get(sizeof(int) * ((size_t)n + 1), st));
  int* off = static_cast<int*>(T.off.get(sizeof(int) * ((size_t)n + 1), st));
  const int* tag = e.d_tag();
  if (ms) SF_HIP(hipEventRecord(T.ev[0], st));
  k_contact_count<<<div_up((long long)n + 1, 256), 256, 0, st>>>(P, S, tag, groupbit, cnt);
  SF_HIP(hipGetLastError());
  exclusive_scan_i32(T.scan_tmp, T.scan_bytes, cnt, off, n + 1, st);
  if (ms) SF_HIP(hipEventRecord(T.ev[1], st));
  SF_HIP(hipMemcpyAsync(T.h_total, off + n, sizeof(int), hipMemcpyDeviceToHost, st));
  SF_HIP(hipStreamSynchronize(st));
  T.launches += 2;
  const long long nrows = *T.h_total;
  if (nrows < 0) fail("compute pair/local: more than 2^31 rows");
  R.n = nrows;
  if (nrows > 0) {
    int* tags = static_cast<int*>(T.tags.get(sizeof(int) * 2 * (size_t)nrows, st));
    double* val = static_cast<double*>(T.vals.get(sizeof(double) * kContactDoubles * (size_t)nrows, st));
    ContactOutCols C;
    C.tag1 = tags;
    C.tag2 = tags + nrows;
    C.val = val;
    C.nrows = (int)nrows;
    if (ms) SF_HIP(hipEventRecord(T.ev[2], st));
    // (plain gran/hooke, GranParams::style 3, runs the Hookean instantiation: the law branches on the style itself)
    style_dispatch(S.gran.style, [&](auto style) {
      constexpr int ST = decltype(style)::value == 2 ? 2 : 1;
      k_contact_rows<ST><<<div_up(n, 256), 256, 0, st>>>(P, S, tag, groupbit, off, C);
    });
    SF_HIP(hipGetLastError());
    T.launches++;
    if (ms) SF_HIP(hipEventRecord(T.ev[3], st));
    R.tag1 = C.tag1;
    R.tag2 = C.tag2;
    R.val = val;
  }
  if (ms) {
    SF_HIP(hipStreamSynchronize(st));
    float a = 0.f, b = 0.f;
    SF_HIP(hipEventElapsedTime(&a, T.ev[0], T.ev[1]));
    if (nrows > 0) SF_HIP(hipEventElapsedTime(&b, T.ev[2], T.ev[3]));
    *ms = (double)a + (double)b;
  }
  return R;
}

int contact_line_stride(const ContactCols& cols)
{
  int stride = 1;
  for (int k = 0; k < cols.n; k++) {
    const int c = cols.c[k];
    stride += 1 + (c == kContactIndex || c == CV_TAG1 || c == CV_TAG2 ? fmt::kMaxD : fmt::kMaxG);
  }
  return stride;
}

void contact_lines_launch(const ContactRows& R, const ContactCols& cols, int stride, char* slots, unsigned long long* len,
                          hipStream_t s)
{
  if (R.n <= 0) return;
  k_contact_lines<<<(unsigned)((R.n + 255) / 256), 256, 0, s>>>(R.tag1, R.tag2, R.val, R.n, cols, stride, slots, len);
}

long long contact_launches(const SfLammps& L)
{
  const ContactSet* S = set_of(L);
  return S ? S->launches : 0;
}

}  // namespace sf

using sf::handle;

extern "C" {

long long sf_lammps_get_contacts(void* ptr, const char* group, long long max, int* tag1, int* tag2, double* values)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  const int groupbit = L.eng.group_bit(group && *group ? group : "all");
  const sf::ContactRows R = sf::contact_rows(L, groupbit);
  if (R.n > 0 && R.n <= max) {
    if (!tag1 || !tag2 || !values) sf::fail("sf_lammps_get_contacts: null argument");
    const size_t n = (size_t)R.n;
    hipStream_t st = L.eng.stream();
    std::vector<double> cols(sf::kContactDoubles * n);
    SF_HIP(hipMemcpyAsync(tag1, R.tag1, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(tag2, R.tag2, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(cols.data(), R.val, sizeof(double) * cols.size(), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    for (size_t r = 0; r < n; r++)   // field-major on the device, row-major for the caller
      for (int c = 0; c < sf::kContactDoubles; c++) values[sf::kContactDoubles * r + c] = cols[(size_t)c * n + r];
  }
  SF_API_END(R.n)
}

int sf_lammps_contact_cost(void* ptr, const char* group, double* out3)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  if (!out3) sf::fail("sf_lammps_contact_cost: null argument");
  const int groupbit = L.eng.group_bit(group && *group ? group : "all");
  double rows_ms = 0.0, text_ms = 0.0;
  const sf::ContactRows R = sf::contact_rows(L, groupbit, &rows_ms);
  sf::dump_local_cost(L, R, &text_ms);
  out3[0] = rows_ms;
  out3[1] = text_ms;
  out3[2] = (double)R.n;
  SF_API_END(0)
}

int sf_lammps_contact_launches(void* ptr, long long* launches)
{
  SF_API_BEGIN
  if (!launches) sf::fail("sf_lammps_contact_launches: null argument");
  *launches = sf::contact_launches(*handle(ptr));
  SF_API_END(0)
}

}  // extern "C"
