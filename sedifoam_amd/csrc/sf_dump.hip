// sf_dump.hip -- `dump ID group custom N file attr...` ([3P] LAMMPS DumpCustom), `dump_modify ID sort id`, `undump ID`:
// the particle snapshots the reference's input scripts write (e.g. xiaocase3/in.lammps: `dump id all custom 1000
// snapshot.bubblemd id type diameter mass x y z vx vy vz`) and its post-processing greps.
//
// A frame is formatted on the GPU, in three launches on the engine's stream:
//   k_dump_lines  one lane per atom: group filter, "%d " / "%g " of every column and "\n" (sf_dump_fmt.h, byte-identical
//                 to glibc) into a fixed-stride slot -- slot = atom index, or tag - 1 with `sort id` (absent tags and atoms
//                 outside the group leave a line of length 0) -- its line length, and the atom count
//   exclusive scan of the line lengths (rocPRIM)
//   k_dump_compact one lane per slot byte: the lines, contiguous
// then an asynchronous copy into one of two pinned host buffers.  A writer thread waits for the copy, writes the header
// and the bytes and flushes; the run goes on meanwhile.  A frame waits only for its buffer's previous write.
//
// `dump ID group local N file index c_ID[k] ...` ([3P] DumpLocal) goes the same way with another first launch: the rows of
// the compute pair/local it names are evaluated (sf_contacts.hip: count, scan, rows) and k_contact_lines, one lane per row,
// fills the slots.  Schedule, `*`, undump, the step-0 frame and the writer are the shared code below.
//
// `c_ID` / `c_ID[k]` columns of a dump custom ([3P] DumpCustom::parse_fields) are the per-atom computes of
// sf_compute_atom.hip: a frame asks for their values (evaluated once per step, whoever asks) and k_dump_lines prints them
// as "%g " from the field-major device columns, between the other columns, sorted or not.
#include <algorithm>
#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/sedifoam_amd.h"
#include "sf_common.h"
#include "sf_compute_atom.h"
#include "sf_compute_ids.h"
#include "sf_compute_parse.h"
#include "sf_contacts.h"
#include "sf_dump.h"
#include "sf_dump_fmt.h"

namespace sf {
namespace {

// the per-atom attributes of a frame: [3P] DumpCustom::parse_fields names; fx..tqz are what sf_dem_get_forces returns
enum Col : unsigned char {
  C_ID, C_TYPE, C_MASS, C_DIAMETER, C_RADIUS, C_X, C_Y, C_Z, C_VX, C_VY, C_VZ, C_FX, C_FY, C_FZ,
  C_OMEGAX, C_OMEGAY, C_OMEGAZ, C_TQX, C_TQY, C_TQZ, C_NCOL
};
const char* const kColName[C_NCOL] = {"id", "type", "mass", "diameter", "radius", "x", "y", "z", "vx", "vy", "vz",
                                      "fx", "fy", "fz", "omegax", "omegay", "omegaz", "tqx", "tqy", "tqz"};
constexpr int kMaxCols = 64;
struct Cols {
  int n;
  unsigned char c[kMaxCols];   // a Col, or C_NCOL + e: column e of XCols
};
// the c_ID / c_ID[k] columns of a frame: one device column of a per-atom compute each, indexed by atom
constexpr int kMaxXCols = 24;
struct XCols {
  const double* p[kMaxXCols];
};

__device__ __forceinline__ double col_value(int c, const double4& x, const double4& v, const double4& w,
                                            const double4& f, const double4& t)
{
  switch (c) {
    case C_MASS: return v.w;
    case C_DIAMETER: return 2.0 * x.w;
    case C_RADIUS: return x.w;
    case C_X: return x.x;
    case C_Y: return x.y;
    case C_Z: return x.z;
    case C_VX: return v.x;
    case C_VY: return v.y;
    case C_VZ: return v.z;
    case C_FX: return f.x;
    case C_FY: return f.y;
    case C_FZ: return f.z;
    case C_OMEGAX: return w.x;
    case C_OMEGAY: return w.y;
    case C_OMEGAZ: return w.z;
    case C_TQX: return t.x;
    case C_TQY: return t.y;
    default: return t.z;
  }
}

// one lane per owned atom.  len[] must hold zeros for the slots no atom writes (sorted frames); err[0] counts atoms whose
// tag has no slot
__global__ __launch_bounds__(256) void k_dump_lines(const double4* xr, const double4* vm, const double4* om,
                                                    const double4* force, const double4* torque, const int* tag,
                                                    const int* type, const int* mask, int n, int groupbit, Cols cols,
                                                    XCols xcols, int sorted, long long nslots, int stride, char* slots,
                                                    unsigned long long* len, unsigned long long* count,
                                                    unsigned long long* err)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n && (mask[i] & groupbit);
  const unsigned long long ballot = __ballot(in);
  if ((threadIdx.x & (warpSize - 1)) == 0 && ballot) atomicAdd(count, (unsigned long long)__popcll(ballot));
  if (i >= n) return;
  const long long slot = sorted ? (long long)tag[i] - 1 : i;
  if (slot < 0 || slot >= nslots) {
    atomicAdd(err, 1ull);
    return;
  }
  if (!in) {
    if (!sorted) len[slot] = 0;
    return;
  }
  const double4 x = xr[i], v = vm[i];
  const double4 w = om[i], f = force[i], t = torque[i];
  char* p0 = slots + slot * (long long)stride;
  char* p = p0;
  for (int k = 0; k < cols.n; k++) {
    const int c = cols.c[k];
    if (c == C_ID) p += fmt::format_d(tag[i], p);
    else if (c == C_TYPE) p += fmt::format_d(type[i], p);
    else if (c >= C_NCOL) p += fmt::format_g(xcols.p[c - C_NCOL][i], p);
    else p += fmt::format_g(col_value(c, x, v, w, f, t), p);
    *p++ = ' ';
  }
  *p++ = '\n';
  len[slot] = (unsigned long long)(p - p0);
}

// the "%d\n" of every int, then the "%g\n" of every double, each in a slot of 16 bytes (sfk_dump_format)
__global__ __launch_bounds__(256) void k_format_values(const int* iv, long long ni, const double* dv, long long nd,
                                                       char* slots, unsigned long long* len)
{
  const long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (k >= ni + nd) return;
  char* p0 = slots + 16 * k;
  char* p = p0;
  p += k < ni ? fmt::format_d(iv[k], p) : fmt::format_g(dv[k - ni], p);
  *p++ = '\n';
  len[k] = (unsigned long long)(p - p0);
}

// one lane per slot byte: the first len[s] bytes of slot s go to out + off[s]
__global__ __launch_bounds__(256) void k_dump_compact(const char* slots, int stride, const unsigned long long* len,
                                                      const unsigned long long* off, long long nslots, char* out)
{
  const long long total = nslots * stride;
  for (long long b = blockIdx.x * (long long)blockDim.x + threadIdx.x; b < total;
       b += (long long)gridDim.x * blockDim.x) {
    const long long s = b / stride;
    const int j = (int)(b - s * stride);
    if ((unsigned long long)j < len[s]) out[off[s] + j] = slots[b];
  }
}

struct Pipeline {
  DeviceScratch slots, len, off, out, scan, small;   // of the format + compact pipeline
  // format nslots slots of `stride` bytes (the caller's kernel `fill` writes them and their lengths into len), then
  // compact; returns the byte count (synchronises the stream once, after the scan) -- the bytes are in out.p.
  // ev: four events around the launches in front of and behind that wait (tools/contact_cost.py)
  template <class Fill>
  size_t run(long long nslots, int stride, bool zero_len, hipStream_t s, Fill fill, unsigned long long* h_small,
             hipEvent_t* ev = nullptr)
  {
    char* d_slots = static_cast<char*>(slots.get((size_t)nslots * stride + 1, s));
    auto* d_len = static_cast<unsigned long long*>(len.get(sizeof(unsigned long long) * (nslots + 1), s));
    auto* d_off = static_cast<unsigned long long*>(off.get(sizeof(unsigned long long) * (nslots + 1), s));
    auto* d_small = static_cast<unsigned long long*>(small.get(4 * sizeof(unsigned long long), s));
    if (ev) SF_HIP(hipEventRecord(ev[0], s));
    SF_HIP(hipMemsetAsync(d_small, 0, 4 * sizeof(unsigned long long), s));
    if (zero_len) SF_HIP(hipMemsetAsync(d_len, 0, sizeof(unsigned long long) * (nslots + 1), s));
    else SF_HIP(hipMemsetAsync(d_len + nslots, 0, sizeof(unsigned long long), s));
    fill(d_slots, d_len, d_small);
    SF_HIP(hipGetLastError());
    size_t need = 0;
    SF_HIP(rocprim::exclusive_scan(nullptr, need, d_len, d_off, 0ull, (size_t)nslots + 1,
                                   rocprim::plus<unsigned long long>(), s));
    void* tmp = scan.get(need, s);
    SF_HIP(rocprim::exclusive_scan(tmp, need, d_len, d_off, 0ull, (size_t)nslots + 1,
                                   rocprim::plus<unsigned long long>(), s));
    if (ev) SF_HIP(hipEventRecord(ev[1], s));
    SF_HIP(hipMemcpyAsync(h_small, d_off + nslots, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SF_HIP(hipMemcpyAsync(h_small + 1, d_small, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    const size_t total = (size_t)h_small[0];
    char* d_out = static_cast<char*>(out.get(total + 1, s));
    if (ev) SF_HIP(hipEventRecord(ev[2], s));
    if (total) {
      const long long bytes = nslots * stride;
      const long long nb = std::min<long long>((bytes + 255) / 256, 1 << 20);
      k_dump_compact<<<(unsigned)nb, 256, 0, s>>>(d_slots, stride, d_len, d_off, nslots, d_out);
      SF_HIP(hipGetLastError());
    }
    if (ev) SF_HIP(hipEventRecord(ev[3], s));
    return total;
  }
};

struct HostBuf {
  char* p = nullptr;
  size_t n = 0;
  hipEvent_t ev = nullptr;
  bool busy = false;   // a queued frame still reads it (guarded by DumpSet::mu)
};

struct Dump {
  std::string id, file, columns;
  int groupbit = 1, every = 1;
  Cols cols{};
  int stride = 1;
  bool sort = false, multifile = false, multiproc = false;
  bool local = false;    // dump local: the rows of `compute` (a compute pair/local), columns lcols
  std::string compute;
  ContactCols lcols{};
  // dump custom: the c_ columns -- column xcol[e] (0-based) of the per-atom compute xid[e] (sf_compute_atom.hip)
  std::vector<std::string> xid;
  std::vector<int> xcol;
  bool gather = false;   // one file written by rank 0 on more than one rank
  long long last = -1;   // the step of the last frame ([3P] Output::last_dump)
  FILE* fp = nullptr;    // the single file (not `*`), opened and truncated by the dump command
  Pipeline pipe;
  char* gathered = nullptr;   // rank 0 of a decomposed run with one file: every rank's bytes (dump_gather)
  size_t gathered_cap = 0;
  HostBuf host[2];
  int next_buf = 0;
  unsigned long long* h_small = nullptr;   // pinned: bytes, atoms, atoms whose tag has no slot
  ~Dump()
  {
    for (HostBuf& h : host) {
      if (h.ev) (void)hipEventDestroy(h.ev);
      if (h.p) (void)hipHostFree(h.p);
    }
    if (h_small) (void)hipHostFree(h_small);
    if (gathered) (void)hipFree(gathered);
    if (fp) fclose(fp);
  }
};

struct Job {
  Dump* d;
  int buf;
  size_t nbytes;
  std::string header, path;   // path empty: d->fp
};

// the dumps of one engine and the thread that writes their frames, in the order they were queued
struct DumpSet {
  std::vector<std::unique_ptr<Dump>> dumps;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> q;
  bool stop = false;
  std::string error;   // the first write error, rethrown by the next dump call
  std::thread th;

  DumpSet() { th = std::thread([this] { loop(); }); }
  ~DumpSet()
  {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
    }
    cv.notify_all();
    th.join();
  }
  void loop()
  {
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [this] { return stop || !q.empty(); });
        if (q.empty()) return;
        j = q.front();
      }
      std::string err;
      if (hipEventSynchronize(j.d->host[j.buf].ev) != hipSuccess) err = "dump: the copy of a frame failed";
      if (err.empty()) {
        FILE* f = j.path.empty() ? j.d->fp : fopen(j.path.c_str(), "w");
        if (!f) err = "Cannot open dump file " + j.path;
        else {
          const bool ok = fwrite(j.header.data(), 1, j.header.size(), f) == j.header.size() &&
                          fwrite(j.d->host[j.buf].p, 1, j.nbytes, f) == j.nbytes && fflush(f) == 0;
          if (!j.path.empty()) fclose(f);
          if (!ok) err = "dump " + j.d->id + ": writing the frame failed";
        }
      }
      {
        std::lock_guard<std::mutex> g(mu);
        j.d->host[j.buf].busy = false;
        q.pop_front();
        if (!err.empty() && error.empty()) error = err;
      }
      cv.notify_all();
    }
  }
  void check_error()
  {
    std::lock_guard<std::mutex> g(mu);
    if (!error.empty()) {
      const std::string e = error;
      error.clear();
      fail("%s", e.c_str());
    }
  }
  void wait_buffer(Dump& d, int b)
  {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return !d.host[b].busy; });
  }
  void drain()
  {
    {
      std::unique_lock<std::mutex> g(mu);
      cv.wait(g, [this] { return q.empty(); });
    }
    check_error();
  }
  Dump* find(const std::string& id)
  {
    for (auto& d : dumps)
      if (d->id == id) return d.get();
    return nullptr;
  }
};

DumpSet* set_of(const SfLammps& L) { return L.dumps.get<DumpSet>(); }
DumpSet& ensure_set(SfLammps& L) { return L.dumps.ensure<DumpSet>(); }

std::string replace_all(std::string s, char c, const std::string& by)
{
  for (size_t k = s.find(c); k != std::string::npos; k = s.find(c, k + by.size())) s.replace(k, 1, by);
  return s;
}

bool ends_with(const std::string& s, const char* suf)
{
  const size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

void write_frame(SfLammps& L, DumpSet& S, Dump& d)
{
  DemEngine& e = L.eng;
  hipStream_t s = e.stream();
  const int n = e.nlocal();
  const long long step = e.nsteps();
  const long long nslots = d.sort ? (long long)e.max_tag() : (long long)n;
  if (!d.h_small) SF_HIP(hipHostMalloc(reinterpret_cast<void**>(&d.h_small), 4 * sizeof(unsigned long long)));
  size_t total = 0;
  unsigned long long natoms = 0;   // (dump local: the rows)
  if (d.local) {
    // the rows are those of the compute's group, evaluated now; the stream is synchronised for their count, and once more
    // below for the byte count
    int groupbit = 1;
    compute_lookup(L, d.compute, nullptr, &groupbit);
    const ContactRows R = contact_rows(L, groupbit);
    natoms = (unsigned long long)R.n;
    if (R.n > 0) {
      const ContactCols cols = d.lcols;
      const int stride = d.stride;
      total = d.pipe.run(R.n, stride, false, s, [&](char* slots, unsigned long long* len, unsigned long long*) {
        contact_lines_launch(R, cols, stride, slots, len, s);
      }, d.h_small);
    }
  } else if (n > 0 && nslots > 0) {
    const int groupbit = d.groupbit, sorted = d.sort ? 1 : 0, stride = d.stride;
    const Cols cols = d.cols;
    XCols xcols{};
    if (!d.xid.empty() && (L.world_size > 1 || L.decomposed || e.nranks() > 1 || e.decomposed()))
      fail("dump %s: c_ columns on one rank only (no decomposed domain)", d.id.c_str());
    for (size_t k = 0; k < d.xid.size(); k++) {
      // (evaluated on this stream, at most once per step however many columns, dumps and queries name the compute)
      int nc = 0;
      const double* val = atom_compute_values(L, d.xid[k], &nc);
      if (d.xcol[k] >= nc) fail("dump %s: compute %s has %d columns", d.id.c_str(), d.xid[k].c_str(), nc);
      xcols.p[k] = val + (size_t)d.xcol[k] * (size_t)n;
    }
    total = d.pipe.run(nslots, stride, d.sort, s, [&](char* slots, unsigned long long* len, unsigned long long* small) {
      k_dump_lines<<<(n + 255) / 256, 256, 0, s>>>(e.d_xr(), e.d_vm(), e.d_om(), e.d_force(), e.d_torque(), e.d_tag(),
                                                   e.d_type(), e.d_mask(), n, groupbit, cols, xcols, sorted, nslots,
                                                   stride, slots, len, small, small + 1);
    }, d.h_small);
    natoms = d.h_small[1];
    if (d.h_small[2])
      fail("dump %s: %llu atoms have a tag outside 1..%d", d.id.c_str(), d.h_small[2], e.max_tag());
  }
  // (the byte count and the atom count are known: the stream was synchronised after the scan)
  const char* src = static_cast<const char*>(d.pipe.out.p);
  if (d.gather) {
    // one file on a decomposed run: rank 0 writes every rank's block, in rank order
    total = dump_gather(L, src, total, natoms, &d.gathered, &d.gathered_cap, &natoms);
    if (L.world_rank != 0) {
      d.last = step;
      return;
    }
    src = d.gathered;
  }
  const int b = d.next_buf;
  d.next_buf ^= 1;
  S.wait_buffer(d, b);
  HostBuf& h = d.host[b];
  if (total + 1 > h.n) {
    if (h.p) SF_HIP(hipHostFree(h.p));
    h.n = total + total / 4 + 4096;
    SF_HIP(hipHostMalloc(reinterpret_cast<void**>(&h.p), h.n));
  }
  if (!h.ev) SF_HIP(hipEventCreateWithFlags(&h.ev, hipEventDisableTiming));
  if (total) SF_HIP(hipMemcpyAsync(h.p, src, total, hipMemcpyDeviceToHost, s));
  SF_HIP(hipEventRecord(h.ev, s));
  // [3P] DumpCustom::header_item (LAMMPS 1Feb14): bounds as "%g %g", flags pp / ff from `boundary`; not checked
  // against a LAMMPS source here
  double lo[3], hi[3];
  int per[3];
  e.box(lo, hi, per);
  // ([3P] DumpLocal::write_header likewise: NUMBER OF ENTRIES / ENTRIES in place of NUMBER OF ATOMS / ATOMS; from memory of
  // LAMMPS 1Feb14 as well, not checked against a LAMMPS source)
  std::vector<char> hb(512 + d.columns.size());
  const int hn = snprintf(hb.data(), hb.size(),
                          d.local ? "ITEM: TIMESTEP\n%lld\nITEM: NUMBER OF ENTRIES\n%llu\nITEM: BOX BOUNDS %s %s %s\n%g %g\n"
                                    "%g %g\n%g %g\nITEM: ENTRIES %s\n"
                                  : "ITEM: TIMESTEP\n%lld\nITEM: NUMBER OF ATOMS\n%llu\nITEM: BOX BOUNDS %s %s %s\n%g %g\n"
                                    "%g %g\n%g %g\nITEM: ATOMS %s\n",
                          step, natoms, per[0] ? "pp" : "ff", per[1] ? "pp" : "ff", per[2] ? "pp" : "ff", lo[0], hi[0],
                          lo[1], hi[1], lo[2], hi[2], d.columns.c_str());
  Job j{&d, b, total, std::string(hb.data(), hn), std::string()};
  if (d.multifile) {
    j.path = replace_all(d.file, '*', std::to_string(step));
    if (d.multiproc) j.path = replace_all(j.path, '%', std::to_string(L.world_rank));
  }
  {
    std::lock_guard<std::mutex> g(S.mu);
    h.busy = true;
    S.q.push_back(std::move(j));
  }
  S.cv.notify_all();
  d.last = step;
}

}  // namespace

// the device formatter on host arrays (sfk_dump_format): "%d\n" of every int, then "%g\n" of every double
void format_values(const double* values, long long nvalues, const int* ints, long long nints, char* out, long long cap,
                   long long* nbytes)
{
  const long long n = nvalues + nints;
  hipStream_t s = nullptr;
  SF_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  struct StreamGuard {
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamDestroy(s); }
  } sg{s};
  DeviceScratch din;
  char* base = static_cast<char*>(din.get(sizeof(double) * nvalues + sizeof(int) * nints + 16, s));
  double* d_val = reinterpret_cast<double*>(base);
  int* d_int = reinterpret_cast<int*>(base + sizeof(double) * nvalues);
  if (nvalues) SF_HIP(hipMemcpyAsync(d_val, values, sizeof(double) * nvalues, hipMemcpyHostToDevice, s));
  if (nints) SF_HIP(hipMemcpyAsync(d_int, ints, sizeof(int) * nints, hipMemcpyHostToDevice, s));
  Pipeline pipe;
  unsigned long long small[4] = {0, 0, 0, 0};
  const size_t total = pipe.run(n, 16, false, s, [&](char* slots, unsigned long long* len, unsigned long long*) {
    k_format_values<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_int, nints, d_val, nvalues, slots, len);
  }, small);
  *nbytes = (long long)total;
  if ((long long)total > cap || !out) sf::fail("sfk_dump_format: %zu bytes do not fit in %lld", total, cap);
  SF_HIP(hipMemcpyAsync(out, pipe.out.p, total, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
}

// dump ID group-ID custom N file attr ...   ([3P] Output::add_dump, DumpCustom::DumpCustom / parse_fields)
void dump_command(SfLammps& L, const std::vector<std::string>& w)
{
  if (w.size() < 6) sf::fail("Illegal dump command");
  const std::string& style = w[3];
  const bool local = style == "local";
  if (style != "custom" && !local)
    sf::fail("Invalid dump style %s (this engine writes dump custom and dump local)", style.c_str());
  if (w.size() < 7) sf::fail("Illegal dump %s command", style.c_str());
  DumpSet& S = ensure_set(L);
  S.check_error();
  if (S.find(w[1])) sf::fail("Reuse of dump ID");
  auto d = std::make_unique<Dump>();
  d->id = w[1];
  d->groupbit = L.eng.group_bit(w[2]);
  char* end = nullptr;
  const long every = std::strtol(w[4].c_str(), &end, 10);
  if (end == w[4].c_str() || *end || every <= 0) sf::fail("Illegal dump command");
  d->every = (int)every;
  d->file = w[5];
  if (ends_with(d->file, ".gz") || ends_with(d->file, ".bin"))
    sf::fail("dump file %s: compressed (.gz) and binary (.bin) dump files are not supported by this engine",
             d->file.c_str());
  d->multifile = d->file.find('*') != std::string::npos;
  d->multiproc = d->file.find('%') != std::string::npos;
  d->gather = L.world_size > 1 && !d->multiproc;
  d->cols.n = 0;
  d->stride = 1;
  d->local = local;
  if (local) {
    // [3P] DumpLocal::parse_fields: index | c_ID | c_ID[k].  The rows are those of ONE compute pair/local -- its group
    // selects them; the dump's own group plays no part, a row has no single atom
    if (d->multiproc || L.world_size > 1 || L.decomposed)
      sf::fail("dump local: one rank and one file only (no %% in the file name, no decomposed domain)");
    std::vector<unsigned char> values;
    for (size_t k = 6; k < w.size(); k++) {
      int c = -1;
      if (w[k] == "index") c = kContactIndex;
      else if (w[k].compare(0, 2, "c_") == 0) {
        std::string id = w[k].substr(2);
        long idx = 0;
        const size_t br = id.find('[');
        if (br != std::string::npos) {
          char* e2 = nullptr;
          idx = std::strtol(id.c_str() + br + 1, &e2, 10);
          if (e2 == id.c_str() + br + 1 || *e2 != ']' || e2[1] || idx < 1)
            sf::fail("Invalid attribute %s in dump local command", w[k].c_str());
          id.resize(br);
        }
        if (!d->compute.empty() && id != d->compute)
          sf::fail("dump local: every c_ column must name the same compute (%s and %s): the rows of two computes are "
                   "not the same rows", d->compute.c_str(), id.c_str());
        fail_if(check_dump_local(compute_shape(L, id), idx, w[k], id));
        if (d->compute.empty()) {
          compute_lookup(L, id, &values, nullptr);
          d->compute = id;
        }
        c = values[idx > 0 ? idx - 1 : 0];
      } else
        sf::fail("Invalid attribute %s in dump local command", w[k].c_str());
      if (d->lcols.n >= kContactMaxCols) sf::fail("Illegal dump local command");
      d->lcols.c[d->lcols.n++] = (unsigned char)c;
      d->columns += (d->columns.empty() ? "" : " ") + w[k];
    }
    if (d->compute.empty())
      sf::fail("Invalid dump style local without a c_ID column: the rows of a dump local are those of its compute "
               "pair/local");
    d->stride = contact_line_stride(d->lcols);
  }
  for (size_t k = 6; k < w.size() && !local; k++) {
    int c = -1;
    for (int q = 0; q < C_NCOL; q++)
      if (w[k] == kColName[q]) c = q;
    if (c < 0 && w[k].compare(0, 2, "c_") == 0) {
      // [3P] DumpCustom::parse_fields: c_ID names a per-atom vector, c_ID[k] a column of a per-atom array
      std::string id;
      long idx = 0;
      const std::string err = parse_compute_column(w[k], "custom", &id, &idx);
      if (!err.empty()) sf::fail("%s", err.c_str());
      fail_if(check_dump_custom(compute_shape(L, id), idx, w[k], id));
      if (L.world_size > 1 || L.decomposed || L.eng.nranks() > 1 || L.eng.decomposed())
        sf::fail("dump custom: c_ columns on one rank only (no decomposed domain)");
      if ((int)d->xid.size() >= kMaxXCols) sf::fail("dump custom: more than %d c_ columns", kMaxXCols);
      c = C_NCOL + (int)d->xid.size();
      d->xid.push_back(id);
      d->xcol.push_back(idx > 0 ? (int)idx - 1 : 0);
    }
    if (c < 0) sf::fail("Invalid attribute %s in dump custom command", w[k].c_str());
    if (d->cols.n >= kMaxCols) sf::fail("Illegal dump custom command");
    d->cols.c[d->cols.n++] = (unsigned char)c;
    d->stride += 1 + (c == C_ID || c == C_TYPE ? fmt::kMaxD : fmt::kMaxG);
    d->columns += (d->columns.empty() ? "" : " ") + w[k];
  }
  if (!d->multifile && !(d->gather && L.world_rank != 0)) {
    // one file for every frame, truncated now (by rank 0 alone when the ranks share it)
    const std::string path = d->multiproc ? replace_all(d->file, '%', std::to_string(L.world_rank)) : d->file;
    d->fp = fopen(path.c_str(), "w");
    if (!d->fp) sf::fail("Cannot open dump file %s", path.c_str());
  }
  S.dumps.push_back(std::move(d));
}

// dump_modify ID sort id | sort off   (the keyword the reference's scripts could need; anything else is refused)
void dump_modify_command(SfLammps& L, const std::vector<std::string>& w)
{
  if (w.size() < 3) sf::fail("Illegal dump_modify command");
  DumpSet* S = set_of(L);
  Dump* d = S ? S->find(w[1]) : nullptr;
  if (!d) sf::fail("Could not find dump_modify ID %s", w[1].c_str());
  if (d->local)
    sf::fail("dump_modify %s on a dump local is not supported by this engine (its rows come in the engine's order: atom "
             "index, then partner tag)", w.size() > 2 ? w[2].c_str() : "");
  for (size_t k = 2; k < w.size(); k += 2) {
    if (w[k] != "sort")
      sf::fail("dump_modify %s is not supported by this engine (only `sort id` is)", w[k].c_str());
    if (k + 1 >= w.size()) sf::fail("Illegal dump_modify command");
    if (w[k + 1] == "off") d->sort = false;
    else if (w[k + 1] == "id") {
      if (d->gather)   // (rank 0 would have to merge the ranks' blocks by tag)
        sf::fail("dump_modify sort id: more than one rank writing a single file is not supported by this engine");
      d->sort = true;
    } else
      sf::fail("dump_modify sort %s is not supported by this engine (only `sort id` is)", w[k + 1].c_str());
  }
}

void undump_command(SfLammps& L, const std::vector<std::string>& w)
{
  if (w.size() != 2) sf::fail("Illegal undump command");
  DumpSet* S = set_of(L);
  Dump* d = S ? S->find(w[1]) : nullptr;
  if (!d) sf::fail("Could not find undump ID %s", w[1].c_str());
  S->drain();   // (its frames are in the file before it goes)
  for (size_t k = 0; k < S->dumps.size(); k++)
    if (S->dumps[k].get() == d) S->dumps.erase(S->dumps.begin() + k);
}

bool dump_active(const SfLammps& L)
{
  const DumpSet* S = set_of(L);
  return S && !S->dumps.empty();
}

long long dump_next_step(const SfLammps& L, long long step)
{
  const DumpSet* S = set_of(L);
  long long best = -1;
  if (!S) return best;
  for (const auto& d : S->dumps) {
    const long long nx = (step / d->every + 1) * d->every;
    if (best < 0 || nx < best) best = nx;
  }
  return best;
}

// [3P] Output::setup / Output::write (LAMMPS 1Feb14 output.cpp): a dump writes at every step that is a multiple of N,
// the setup of a run included, but never twice at one step (last_dump).  Restated from the LAMMPS documentation of
// `dump` and `run`; no LAMMPS source was at hand to check it against.
void dump_write_due(SfLammps& L)
{
  DumpSet* S = set_of(L);
  if (!S) return;
  S->check_error();
  const long long step = L.eng.nsteps();
  for (auto& d : S->dumps)
    if (step % d->every == 0 && d->last != step) write_frame(L, *S, *d);
}

void dump_drain(SfLammps& L)
{
  if (DumpSet* S = set_of(L)) S->drain();
}

bool dump_uses_compute(const SfLammps& L, const std::string& id)
{
  const DumpSet* S = set_of(L);
  if (!S) return false;
  for (const auto& d : S->dumps)
    if ((d->local && d->compute == id) || std::find(d->xid.begin(), d->xid.end(), id) != d->xid.end()) return true;
  return false;
}

size_t dump_local_cost(SfLammps& L, const ContactRows& R, double* ms)
{
  *ms = 0.0;
  if (R.n <= 0) return 0;
  hipStream_t s = L.eng.stream();
  ContactCols cols;
  cols.n = 0;
  cols.c[cols.n++] = kContactIndex;
  for (int c = 0; c < CV_COUNT; c++) cols.c[cols.n++] = (unsigned char)c;
  const int stride = contact_line_stride(cols);
  hipEvent_t ev[4];
  for (hipEvent_t& e : ev) SF_HIP(hipEventCreate(&e));
  struct EvGuard {
    hipEvent_t* ev;
    ~EvGuard()
    {
      for (int k = 0; k < 4; k++) (void)hipEventDestroy(ev[k]);
    }
  } guard{ev};
  Pipeline pipe;
  unsigned long long small[4] = {0, 0, 0, 0};
  const size_t total = pipe.run(R.n, stride, false, s, [&](char* slots, unsigned long long* len, unsigned long long*) {
    contact_lines_launch(R, cols, stride, slots, len, s);
  }, small, ev);
  SF_HIP(hipStreamSynchronize(s));
  float a = 0.f, b = 0.f;
  SF_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
  SF_HIP(hipEventElapsedTime(&b, ev[2], ev[3]));
  *ms = (double)a + (double)b;
  return total;
}

}  // namespace sf

extern "C" {

int sfk_dump_format(const double* values, long long nvalues, const int* ints, long long nints, char* out,
                    long long cap, long long* nbytes)
{
  SF_API_BEGIN
  if (nvalues < 0 || nints < 0 || (nvalues && !values) || (nints && !ints) || !nbytes)
    sf::fail("sfk_dump_format: bad arguments");
  const long long n = nvalues + nints;
  *nbytes = 0;
  if (n > 0) sf::format_values(values, nvalues, ints, nints, out, cap, nbytes);
  SF_API_END(0)
}

}  // extern "C"
