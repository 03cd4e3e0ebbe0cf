// sf_restart.hip -- checkpoints: `write_restart FILE`, `restart N ...`, `read_restart FILE`.
//   * the file (format version 1; sedifoam_amd/restart.py is its executable specification, DESIGN.md section 10 its table)
//   * DemEngine::restart_pack: the owned atoms in tag order, every touching contact once (from the lower tag), the wall
//     rows -- counted, scanned and filled on the device into component-major columns
//   * DemEngine::restart_unpack: the columns go up as they are; a kernel expands the CSR contacts into the partner rows
//     of both sides, which the first list build re-injects by partner tag like the rows of a migrated atom
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include <unistd.h>

#include "sf_dem.h"
#include "sf_dump.h"
#include "sf_handles.h"
#include "sf_restart.h"
#include "sf_thermo.h"

namespace sf {

// ------------------------------------------------------------------------------------------------
// the file
// ------------------------------------------------------------------------------------------------
namespace {

constexpr char kMagic[8] = {'S', 'F', 'R', 'E', 'S', 'T', 'R', 'T'};
constexpr uint32_t kVersion = 1, kBom = 0x01020304u;
constexpr size_t kFixedBytes = 152, kGroupBytes = 64, kWallBytes = 64, kSectionBytes = 48;
constexpr uint32_t kI32 = 1, kF64 = 2;

// CRC-32 (IEEE 802.3, the one zlib computes), eight bytes per step
struct CrcTable {
  uint32_t t[8][256];
  CrcTable()
  {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; i++)
      for (int k = 1; k < 8; k++) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xff];
  }
};

uint32_t crc32(const void* data, size_t n)
{
  static const CrcTable T;
  const unsigned char* p = static_cast<const unsigned char*>(data);
  uint32_t c = 0xffffffffu;
  while (n >= 8) {
    uint32_t a, b;
    memcpy(&a, p, 4);
    memcpy(&b, p + 4, 4);
    a ^= c;
    c = T.t[7][a & 0xff] ^ T.t[6][(a >> 8) & 0xff] ^ T.t[5][(a >> 16) & 0xff] ^ T.t[4][a >> 24] ^ T.t[3][b & 0xff] ^
        T.t[2][(b >> 8) & 0xff] ^ T.t[1][(b >> 16) & 0xff] ^ T.t[0][b >> 24];
    p += 8;
    n -= 8;
  }
  while (n--) c = T.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
  return c ^ 0xffffffffu;
}

struct Section {
  std::string name;
  uint32_t dtype;
  const void* data;
  size_t nbytes;
};

size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

template <class T>
void put(std::vector<unsigned char>& b, T v)
{
  unsigned char raw[sizeof(T)];
  memcpy(raw, &v, sizeof(T));
  b.insert(b.end(), raw, raw + sizeof(T));
}

void put_name(std::vector<unsigned char>& b, const std::string& s, size_t width, const char* what)
{
  if (s.size() >= width) fail("write_restart: %s %s does not fit %d bytes", what, s.c_str(), (int)width - 1);
  b.insert(b.end(), s.begin(), s.end());
  b.insert(b.end(), width - s.size(), 0);
}

std::vector<Section> sections_of(const RestartData& d, std::vector<std::string>& names)
{
  std::vector<Section> s;
  auto I = [&](const char* n, const std::vector<int>& v) { s.push_back({n, kI32, v.data(), v.size() * sizeof(int)}); };
  auto D = [&](const char* n, const std::vector<double>& v) { s.push_back({n, kF64, v.data(), v.size() * sizeof(double)}); };
  I("tag", d.tag); I("type", d.type); I("mask", d.mask); I("foamCpuId", d.foam);
  D("x", d.x); D("radius", d.radius); D("v", d.v); D("rmass", d.rmass); D("omega", d.omega);
  D("fdrag", d.fdrag); D("DuDt", d.DuDt); D("vOld", d.vOld);
  I("contact_count", d.ccount); I("contact_partner", d.cpartner); D("contact_shear", d.cshear);
  names.clear();
  for (size_t k = 0; k < d.walls.size(); k++) {
    names.push_back("wall" + std::to_string(k) + ".tag");
    names.push_back("wall" + std::to_string(k) + ".shear");
  }
  for (size_t k = 0; k < d.walls.size(); k++) {
    I(names[2 * k].c_str(), d.walls[k].tag);
    D(names[2 * k + 1].c_str(), d.walls[k].shear);
  }
  return s;
}

template <class T>
T get(const unsigned char* p)
{
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
}

std::string cstr(const unsigned char* p, size_t width)
{
  size_t n = 0;
  while (n < width && p[n]) n++;
  return std::string(reinterpret_cast<const char*>(p), n);
}

}  // namespace

void restart_file_write(const std::string& path, const RestartData& d)
{
  const size_t n = (size_t)d.natoms, nc = (size_t)d.ncontacts;
  if (d.tag.size() != n || d.type.size() != n || d.mask.size() != n || d.foam.size() != n || d.ccount.size() != n ||
      d.x.size() != 3 * n || d.radius.size() != n || d.v.size() != 3 * n || d.rmass.size() != n || d.omega.size() != 3 * n ||
      d.fdrag.size() != 3 * n || d.DuDt.size() != 3 * n || d.vOld.size() != 3 * n || d.cpartner.size() != nc ||
      d.cshear.size() != 3 * nc)
    fail("write_restart: inconsistent section sizes");
  std::vector<std::string> names;
  const std::vector<Section> secs = sections_of(d, names);
  const size_t header_bytes =
      kFixedBytes + kGroupBytes * d.groups.size() + kWallBytes * d.walls.size() + kSectionBytes * secs.size() + 8;
  size_t off = header_bytes;
  std::vector<unsigned char> table;
  for (const Section& s : secs) {
    put_name(table, s.name, 24, "section");
    put<uint32_t>(table, s.dtype);
    put<uint32_t>(table, crc32(s.data, s.nbytes));
    put<uint64_t>(table, off);
    put<uint64_t>(table, s.nbytes);
    off += pad8(s.nbytes);
  }
  std::vector<unsigned char> h;
  h.insert(h.end(), kMagic, kMagic + 8);
  put<uint32_t>(h, kVersion);
  put<uint32_t>(h, kBom);
  put<uint64_t>(h, header_bytes);
  put<uint64_t>(h, off);
  put<int64_t>(h, d.natoms);
  put<int64_t>(h, d.ncontacts);
  put<int64_t>(h, d.step);
  put<int64_t>(h, d.max_tag);
  put<double>(h, d.dt);
  for (int k = 0; k < 3; k++) put<double>(h, d.lo[k]);
  for (int k = 0; k < 3; k++) put<double>(h, d.hi[k]);
  for (int k = 0; k < 3; k++) put<int32_t>(h, d.periodic[k]);
  put<int32_t>(h, d.units_lj ? 1 : 0);
  put<uint32_t>(h, (uint32_t)d.groups.size());
  put<uint32_t>(h, (uint32_t)d.walls.size());
  put<uint32_t>(h, (uint32_t)secs.size());
  put<uint32_t>(h, crc32(h.data(), h.size()));
  for (const auto& g : d.groups) {
    put_name(h, g.first, 60, "group");
    put<int32_t>(h, g.second);
  }
  for (const RestartWall& w : d.walls) {
    put_name(h, w.id, 56, "fix ID");
    put<int64_t>(h, (int64_t)w.tag.size());
  }
  h.insert(h.end(), table.begin(), table.end());
  put<uint32_t>(h, crc32(h.data(), h.size()));
  put<uint32_t>(h, 0);
  if (h.size() != header_bytes) fail("write_restart: header size %zu != %zu", h.size(), header_bytes);

  const std::string tmp = path + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) fail("Cannot open restart file %s: %s", tmp.c_str(), strerror(errno));
  static const unsigned char zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool ok = fwrite(h.data(), 1, h.size(), f) == h.size();
  for (const Section& s : secs) {
    ok = ok && (s.nbytes == 0 || fwrite(s.data, 1, s.nbytes, f) == s.nbytes);
    const size_t padn = pad8(s.nbytes) - s.nbytes;
    ok = ok && (padn == 0 || fwrite(zeros, 1, padn, f) == padn);
  }
  ok = ok && fflush(f) == 0 && fsync(fileno(f)) == 0;   // (on the disk before the rename: a reset must not leave a short file)
  int err = ok ? 0 : errno;
  if (fclose(f) != 0) {
    if (ok) err = errno;
    ok = false;
  }
  if (!ok) {
    remove(tmp.c_str());
    fail("Cannot write restart file %s: %s", tmp.c_str(), strerror(err));
  }
  if (rename(tmp.c_str(), path.c_str()) != 0) {
    const int e2 = errno;
    remove(tmp.c_str());
    fail("Cannot rename restart file %s to %s: %s", tmp.c_str(), path.c_str(), strerror(e2));
  }
}

void restart_file_read(const std::string& path, RestartData& d)
{
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) fail("Cannot open restart file %s", path.c_str());
  std::vector<unsigned char> b;
  {
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    b.resize(sz > 0 ? (size_t)sz : 0);
    const size_t got = b.empty() ? 0 : fread(b.data(), 1, b.size(), f);
    fclose(f);
    if (got != b.size()) fail("Cannot read restart file %s", path.c_str());
  }
  const char* P = path.c_str();
  auto truncated = [&]() { fail("Restart file %s is truncated", P); };
  auto corrupted = [&]() { fail("Restart file %s is corrupted", P); };
  if (b.size() < 16) truncated();
  if (memcmp(b.data(), kMagic, 8) != 0) fail("%s is not a sedifoam_amd restart file (bad magic)", P);
  const uint32_t version = get<uint32_t>(&b[8]), bom = get<uint32_t>(&b[12]);
  if (bom != kBom) {
    if (bom == 0x04030201u) fail("Restart file %s was written with the other byte order", P);
    corrupted();
  }
  if (version > kVersion || version < 1)
    fail("Restart file %s has format version %u, this code reads up to version %u", P, version, kVersion);
  if (b.size() < kFixedBytes) truncated();
  if (get<uint32_t>(&b[kFixedBytes - 4]) != crc32(b.data(), kFixedBytes - 4)) corrupted();
  const uint64_t header_bytes = get<uint64_t>(&b[16]), file_bytes = get<uint64_t>(&b[24]);
  d = RestartData();
  d.natoms = get<int64_t>(&b[32]);
  d.ncontacts = get<int64_t>(&b[40]);
  d.step = get<int64_t>(&b[48]);
  d.max_tag = get<int64_t>(&b[56]);
  d.dt = get<double>(&b[64]);
  for (int k = 0; k < 3; k++) {
    d.lo[k] = get<double>(&b[72 + 8 * k]);
    d.hi[k] = get<double>(&b[96 + 8 * k]);
    d.periodic[k] = get<int32_t>(&b[120 + 4 * k]);
  }
  d.units_lj = get<int32_t>(&b[132]);
  const uint32_t ngroups = get<uint32_t>(&b[136]), nwalls = get<uint32_t>(&b[140]), nsec = get<uint32_t>(&b[144]);
  if (header_bytes != kFixedBytes + kGroupBytes * ngroups + kWallBytes * nwalls + kSectionBytes * nsec + 8 ||
      d.natoms < 0 || d.ncontacts < 0 || d.natoms > 0x7fffffff || d.ncontacts > 0x7fffffff)
    corrupted();
  if (b.size() < header_bytes) truncated();
  if (get<uint32_t>(&b[header_bytes - 8]) != crc32(b.data(), header_bytes - 8)) corrupted();
  if (b.size() < file_bytes) truncated();
  if (b.size() > file_bytes) corrupted();
  size_t p = kFixedBytes;
  for (uint32_t g = 0; g < ngroups; g++, p += kGroupBytes) d.groups.push_back({cstr(&b[p], 60), get<int32_t>(&b[p + 60])});
  std::vector<int64_t> wcount;
  for (uint32_t w = 0; w < nwalls; w++, p += kWallBytes) {
    RestartWall W;
    W.id = cstr(&b[p], 56);
    wcount.push_back(get<int64_t>(&b[p + 56]));
    if (wcount.back() < 0 || wcount.back() > d.natoms) corrupted();
    d.walls.push_back(W);
  }
  const size_t n = (size_t)d.natoms, nc = (size_t)d.ncontacts;
  d.tag.resize(n); d.type.resize(n); d.mask.resize(n); d.foam.resize(n); d.ccount.resize(n);
  d.x.resize(3 * n); d.radius.resize(n); d.v.resize(3 * n); d.rmass.resize(n); d.omega.resize(3 * n);
  d.fdrag.resize(3 * n); d.DuDt.resize(3 * n); d.vOld.resize(3 * n);
  d.cpartner.resize(nc); d.cshear.resize(3 * nc);
  for (uint32_t w = 0; w < nwalls; w++) {
    d.walls[w].tag.resize((size_t)wcount[w]);
    d.walls[w].shear.resize(3 * (size_t)wcount[w]);
  }
  std::vector<std::string> names;
  const std::vector<Section> secs = sections_of(d, names);
  // (a later version may append sections behind these; the ones of version 1 keep their names, types and order)
  if (secs.size() != nsec) corrupted();
  size_t end = header_bytes;
  for (const Section& s : secs) {
    if (cstr(&b[p], 24) != s.name || get<uint32_t>(&b[p + 24]) != s.dtype) corrupted();
    const uint32_t crc = get<uint32_t>(&b[p + 28]);
    const uint64_t off = get<uint64_t>(&b[p + 32]), nb = get<uint64_t>(&b[p + 40]);
    if (nb != s.nbytes || off != end || off + nb > b.size()) corrupted();
    if (crc32(&b[0] + off, nb) != crc) corrupted();
    if (nb) memcpy(const_cast<void*>(s.data), &b[0] + off, nb);
    end = off + pad8(nb);
    p += kSectionBytes;
  }
  for (size_t i = 1; i < n; i++)
    if (d.tag[i] <= d.tag[i - 1]) corrupted();
  long long sum = 0;
  for (size_t i = 0; i < n; i++) {
    if (d.ccount[i] < 0) corrupted();
    sum += d.ccount[i];
  }
  if (sum != d.ncontacts) corrupted();
  for (size_t i = 0, e = 0; i < n; i++)   // partners: higher than the atom's own tag, ascending within the atom
    for (int k = 0, prev = d.tag[i]; k < d.ccount[i]; k++, e++) {
      if (d.cpartner[e] <= prev) corrupted();
      prev = d.cpartner[e];
    }
  for (const RestartWall& w : d.walls)
    for (size_t i = 1; i < w.tag.size(); i++)
      if (w.tag[i] <= w.tag[i - 1]) corrupted();
}

// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------
namespace {

struct DevBuf {   // scratch of one checkpoint (a checkpoint is rare: allocated and freed per call)
  void* p = nullptr;
  explicit DevBuf(size_t bytes) { SF_HIP(hipMalloc(&p, bytes ? bytes : 8)); }
  ~DevBuf() { (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

__global__ __launch_bounds__(256) void k_rst_keys(const int* tag, int n, unsigned* keys, int* idx)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = (unsigned)tag[i];
  idx[i] = i;
}

// per atom of rank r in tag order: the contacts it writes (touching partners with a higher tag: a partner row holds a
// tag >= 0 only where the touch bit is set) and, per wall, whether it has a row.  cnt: [1 + nwalls][n + 1], the last
// element of every row stays zero so that the exclusive scan ends in the total
__global__ __launch_bounds__(256) void k_rst_count(const int* order, int n, const int* tag, const int* numneigh,
                                                   const int* ptag, size_t cap, int M, const unsigned char* wtouch,
                                                   int nwalls, int* cnt)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int i = order[r];
  int c = 0;
  if (numneigh) {
    const int nn = min(numneigh[i], M), t = tag[i];
    // (two touching images of one partner share a tag: one entry, as the fill kernel's strictly ascending walk finds)
    for (int s = 0; s < nn; s++) {
      const int p = ptag[(size_t)s * cap + i];
      bool fresh = p > t;
      for (int u = 0; u < s && fresh; u++) fresh = ptag[(size_t)u * cap + i] != p;
      c += fresh ? 1 : 0;
    }
  }
  cnt[r] = c;
  const unsigned wt = nwalls ? wtouch[i] : 0u;
  for (int w = 0; w < nwalls; w++) cnt[(size_t)(w + 1) * (n + 1) + r] = (wt >> w) & 1u;
}

struct RstAtomCols {   // component-major output columns, n elements each
  int *tag, *type, *mask, *foam;
  double *x, *radius, *v, *rmass, *omega, *fdrag, *DuDt, *vOld;
};

// lane r gathers the records of the atom of rank r and stores one element of every column: consecutive lanes write
// consecutive addresses of each column (whole lines), the gathers are the scattered side
__global__ __launch_bounds__(256) void k_rst_atoms(const int* order, int n, const double4* xr, const double4* vm,
                                                   const double4* om, const int* tag, const int* type, const int* mask,
                                                   const int* foam, const double* fdrag, const double* DuDt,
                                                   const double* vOld, size_t cap, RstAtomCols C)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int i = order[r];
  const double4 x = xr[i], v = vm[i], w = om[i];
  C.tag[r] = tag[i];
  C.type[r] = type[i];
  C.mask[r] = mask[i];
  C.foam[r] = foam[i];
  C.x[r] = x.x; C.x[(size_t)n + r] = x.y; C.x[2 * (size_t)n + r] = x.z;
  C.radius[r] = x.w;
  C.v[r] = v.x; C.v[(size_t)n + r] = v.y; C.v[2 * (size_t)n + r] = v.z;
  C.rmass[r] = v.w;
  C.omega[r] = w.x; C.omega[(size_t)n + r] = w.y; C.omega[2 * (size_t)n + r] = w.z;
  for (int c = 0; c < 3; c++) {
    C.fdrag[(size_t)c * n + r] = fdrag[(size_t)c * cap + i];
    C.DuDt[(size_t)c * n + r] = DuDt[(size_t)c * cap + i];
    C.vOld[(size_t)c * n + r] = vOld[(size_t)c * cap + i];
  }
}

// the contacts of the atom of rank r go to [off[r], off[r + 1]), partners in ascending tag order (selection by repeated
// minimum: a row has a handful of them).  Neighbouring lanes fill neighbouring ranges, so a wave's stores cover a
// contiguous stretch of each column
__global__ __launch_bounds__(256) void k_rst_contacts(const int* order, int n, const int* tag, const int* numneigh,
                                                      const int* ptag, const double* shear, size_t cap, int M,
                                                      const int* off, int nc, int* cpartner, double* cshear)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int first = off[r], count = off[r + 1] - first;
  if (count <= 0) return;
  const int i = order[r];
  const int nn = min(numneigh[i], M);
  int prev = tag[i];
  for (int k = 0; k < count; k++) {
    int best = 0x7fffffff, slot = -1;
    for (int s = 0; s < nn; s++) {
      const int t = ptag[(size_t)s * cap + i];
      if (t > prev && t < best) {
        best = t;
        slot = s;
      }
    }
    const int e = first + k;
    if (slot < 0 || e >= nc) return;   // (two touching images of one partner share a tag: the first one found is kept)
    cpartner[e] = best;
    const size_t src = (size_t)(3 * slot) * cap + i;
    cshear[e] = shear[src];
    cshear[(size_t)nc + e] = shear[src + cap];
    cshear[2 * (size_t)nc + e] = shear[src + 2 * cap];
    prev = best;
  }
}

__global__ __launch_bounds__(256) void k_rst_wall(const int* order, int n, const int* tag, const double* wshear3,
                                                  size_t cap, const int* woff, int m, int* wtag, double* wsh)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int e = woff[r];
  if (woff[r + 1] == e || e >= m) return;
  const int i = order[r];
  wtag[e] = tag[i];
  for (int c = 0; c < 3; c++) wsh[(size_t)c * m + e] = wshear3[(size_t)c * cap + i];
}

struct RstFileCols {   // the columns of a file on the device, N atoms
  const int *tag, *type, *mask, *foam;
  const double *x, *radius, *v, *rmass, *omega, *fdrag, *DuDt, *vOld;
};

// atom k of this rank = atom keep[k] of the file -> slot first + k
__global__ __launch_bounds__(256) void k_rst_unpack_atoms(const int* keep, int nkeep, int N, RstFileCols F, int first,
                                                          double4* xr, double4* vm, double4* om, int* tag, int* type,
                                                          int* mask, int* foam, double* fdrag, double* DuDt, double* vOld,
                                                          int* numneigh, unsigned char* wtouch, size_t cap)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeep) return;
  const int r = keep[k], i = first + k;
  const size_t n = (size_t)N;
  xr[i] = {F.x[r], F.x[n + r], F.x[2 * n + r], F.radius[r]};
  vm[i] = {F.v[r], F.v[n + r], F.v[2 * n + r], F.rmass[r]};
  om[i] = {F.omega[r], F.omega[n + r], F.omega[2 * n + r], 0.0};   // (.w, the frozen mark, follows the mask: mark_frozen)
  tag[i] = F.tag[r];
  type[i] = F.type[r];
  mask[i] = F.mask[r];
  foam[i] = F.foam[r];
  for (int c = 0; c < 3; c++) {
    fdrag[(size_t)c * cap + i] = F.fdrag[(size_t)c * n + r];
    DuDt[(size_t)c * cap + i] = F.DuDt[(size_t)c * n + r];
    vOld[(size_t)c * cap + i] = F.vOld[(size_t)c * n + r];
  }
  numneigh[i] = 0;
  wtouch[i] = 0;
}

__device__ __forceinline__ int rst_find(const int* sorted, int n, int key)   // position of key in an ascending array, -1: absent
{
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && sorted[lo] == key) ? lo : -1;
}

// contact e of the file (CSR: off[N + 1] over the atoms in tag order) -> a partner row on each side this rank keeps:
// the lower tag's as saved, the higher tag's negated.  fill = 0 counts the rows only (numneigh), fill = 1 writes them
__global__ __launch_bounds__(256) void k_rst_expand(int nc, int N, const int* off, const int* ftag, const int* cpartner,
                                                    const double* cshear, const int* loc, int first, int fill, int M,
                                                    int* numneigh, int* ptag, double* shear, size_t cap)
{
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nc) return;
  int lo = 0, hi = N;   // the last r with off[r] <= e
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= e) lo = mid;
    else hi = mid;
  }
  const int ri = lo, tj = cpartner[e], rj = rst_find(ftag, N, tj);
  const int side[2] = {loc[ri], rj >= 0 ? loc[rj] : -1};
  const int other[2] = {tj, ftag[ri]};
  for (int q = 0; q < 2; q++) {
    if (side[q] < 0) continue;
    const int i = first + side[q];
    const int s = atomicAdd(&numneigh[i], 1);
    if (!fill || s >= M) continue;
    const double sg = q ? -1.0 : 1.0;
    ptag[(size_t)s * cap + i] = other[q];
    for (int c = 0; c < 3; c++) shear[(size_t)(3 * s + c) * cap + i] = sg * cshear[(size_t)c * nc + e];
  }
}

__global__ __launch_bounds__(256) void k_rst_wall_rows(const int* wtag, const double* wsh, int m, const int* tag, int nlocal,
                                                       int w, double* wshear, unsigned char* wtouch, size_t cap)
{
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int i = rst_find(tag, nlocal, wtag[e]);   // (the owned atoms are still in the file's order: ascending tags)
  if (i < 0) return;                              // an atom of another rank
  for (int c = 0; c < 3; c++) wshear[(size_t)(3 * w + c) * cap + i] = wsh[(size_t)c * m + e];
  wtouch[i] |= (unsigned char)(1u << w);          // (one lane per atom and launch: a plain read-modify-write)
}

template <class T>
void down(std::vector<T>& dst, const T* src, size_t n, hipStream_t s)
{
  dst.resize(n);
  if (n) SF_HIP(hipMemcpyAsync(dst.data(), src, sizeof(T) * n, hipMemcpyDeviceToHost, s));
}

template <class T>
T* up(DevBuf& b, const std::vector<T>& src, hipStream_t s)
{
  if (!src.empty()) SF_HIP(hipMemcpyAsync(b.p, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, s));
  return b.as<T>();
}

}  // namespace

// One checkpoint block of this rank in a persistent device buffer (no allocation per checkpoint once it has grown):
//   long long hdr[16] = {n, nc, max_tag, nwalls, m_0 .. m_5} | int32: tag type mask foamCpuId contact_count [n each],
//   contact_partner [nc], wall tags [m_w each] (padded to 8 bytes) | f64: x radius v rmass omega fdrag DuDt vOld
//   [3 n / n], contact_shear [3 nc], wall shear [3 m_w each] -- atoms in ascending tag order, columns component-major.
// Returns the byte count; *blob stays valid until the next call.
size_t DemEngine::restart_pack_device(const char** blob, double* pack_ms)
{
  const int n = nlocal_;
  const size_t N = (size_t)n;
  const int nrow = 1 + nwalls_;
  auto grow = [&](int which, size_t bytes) {
    if (bytes > rst_cap_[which]) {
      sync();
      if (rst_buf_[which]) SF_HIP(hipFree(rst_buf_[which]));
      rst_cap_[which] = bytes + bytes / 4 + 4096;
      SF_HIP(hipMalloc(&rst_buf_[which], rst_cap_[which]));
    }
    return rst_buf_[which];
  };
  if (pack_ms) SF_HIP(hipEventRecord(ev0_, stream_));
  long long* hdr = rst_hdr_;
  for (int k = 0; k < 16; k++) hdr[k] = 0;
  hdr[0] = n;
  hdr[2] = max_tag_;
  hdr[3] = nwalls_;
  int* cnt = nullptr;
  int* offs = nullptr;
  const int nb = div_up(n > 0 ? n : 1, 256);
  const int M = max_neigh_used_;
  const bool rows = (have_list_ || hist_rows_) && M > 0;
  const int hb = cur_ ^ 1;
  const int* order = perm_alt_.as<int>();
  if (n) {
    // 1. the history as partner rows (numneigh, partner tag, shear per side) in the ping-pong buffer the sub-steps are
    //    not using: from the live list, or as read_restart left them
    if (have_list_ && M > 0) {
      restart_partner_rows(M);
      restart_launches_++;
    } else if (hist_rows_ && hist_buf_ != hb)
      fail("write_restart: the partner rows of read_restart are not where they were left");
    // 2. tag order, counts, offsets
    cnt = static_cast<int*>(grow(0, sizeof(int) * nrow * (N + 1)));
    offs = static_cast<int*>(grow(1, sizeof(int) * nrow * (N + 1)));
    k_rst_keys<<<nb, 256, 0, stream_>>>(tag_.as<int>(), n, keys_.as<unsigned>(), perm_.as<int>());
    sort_pairs_u32(sort_tmp_, sort_tmp_bytes_, keys_.as<unsigned>(), keys_alt_.as<unsigned>(), perm_.as<int>(),
                   perm_alt_.as<int>(), n, 32, stream_);
    SF_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * nrow * (N + 1), stream_));
    k_rst_count<<<nb, 256, 0, stream_>>>(order, n, tag_.as<int>(), rows ? numneigh_.as<int>() : nullptr, ptag_.as<int>(),
                                         cap_, M, wtouch_.as<unsigned char>(), nwalls_, cnt);
    for (int q = 0; q < nrow; q++)
      exclusive_scan_i32(sort_tmp_, sort_tmp_bytes_, cnt + (size_t)q * (N + 1), offs + (size_t)q * (N + 1), n + 1, stream_);
    restart_launches_ += 3 + nrow;
    int total[1 + kMaxWalls];
    for (int q = 0; q < nrow; q++)
      SF_HIP(hipMemcpyAsync(&total[q], offs + (size_t)q * (N + 1) + N, sizeof(int), hipMemcpyDeviceToHost, stream_));
    sync();
    hdr[1] = total[0];
    for (int w = 0; w < nwalls_; w++) hdr[4 + w] = total[1 + w];
  }
  const size_t nc = (size_t)hdr[1];
  size_t msum = 0;
  for (int w = 0; w < nwalls_; w++) msum += (size_t)hdr[4 + w];
  const size_t nint = (5 * N + nc + msum + 1) & ~(size_t)1, ndbl = 20 * N + 3 * nc + 3 * msum;
  const size_t bytes = 128 + 4 * nint + 8 * ndbl;
  char* B = static_cast<char*>(grow(2, bytes));
  SF_HIP(hipMemcpyAsync(B, hdr, 128, hipMemcpyHostToDevice, stream_));
  if (n) {
    int* I = reinterpret_cast<int*>(B + 128);
    double* D = reinterpret_cast<double*>(B + 128 + 4 * nint);
    SF_HIP(hipMemsetAsync(I + 5 * N, 0, 4 * (nint - 5 * N), stream_));   // (CSR partners, wall tags, the pad word)
    RstAtomCols C;
    C.tag = I; C.type = I + N; C.mask = I + 2 * N; C.foam = I + 3 * N;
    C.x = D; C.radius = C.x + 3 * N; C.v = C.radius + N; C.rmass = C.v + 3 * N; C.omega = C.rmass + N;
    C.fdrag = C.omega + 3 * N; C.DuDt = C.fdrag + 3 * N; C.vOld = C.DuDt + 3 * N;
    k_rst_atoms<<<nb, 256, 0, stream_>>>(order, n, xr_[cur_].as<double4>(), vm_[cur_].as<double4>(), om_[cur_].as<double4>(),
                                         tag_.as<int>(), type_.as<int>(), mask_.as<int>(), foamCpuId_.as<int>(),
                                         fdrag_.as<double>(), DuDt_.as<double>(), vOld_.as<double>(), cap_, C);
    SF_HIP(hipMemcpyAsync(I + 4 * N, cnt, sizeof(int) * N, hipMemcpyDeviceToDevice, stream_));
    restart_launches_++;
    int* cp = I + 5 * N;
    double* cs = D + 20 * N;
    if (nc) {
      SF_HIP(hipMemsetAsync(cs, 0, sizeof(double) * 3 * nc, stream_));
      k_rst_contacts<<<nb, 256, 0, stream_>>>(order, n, tag_.as<int>(), numneigh_.as<int>(), ptag_.as<int>(),
                                              shear_[hb].as<double>(), cap_, M, offs, (int)nc, cp, cs);
      restart_launches_++;
    }
    int* wt = cp + nc;
    double* ws = cs + 3 * nc;
    for (int w = 0; w < nwalls_; w++) {
      const size_t m = (size_t)hdr[4 + w];
      if (m) {
        k_rst_wall<<<nb, 256, 0, stream_>>>(order, n, tag_.as<int>(), wshear_.as<double>() + (size_t)(3 * w) * cap_, cap_,
                                            offs + (size_t)(w + 1) * (N + 1), (int)m, wt, ws);
        restart_launches_++;
      }
      wt += m;
      ws += 3 * m;
    }
  }
  if (pack_ms) {
    SF_HIP(hipEventRecord(ev1_, stream_));
    sync();
    float ms = 0.f;
    SF_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
    *pack_ms = ms;
  }
  *blob = B;
  return bytes;
}

void DemEngine::restart_describe(RestartData& out) const
{
  out.step = nsteps_;
  out.dt = dt_;
  for (int k = 0; k < 3; k++) {
    out.lo[k] = boxlo_[k];
    out.hi[k] = boxhi_[k];
    out.periodic[k] = periodic_[k];
  }
  out.groups.clear();
  for (const auto& g : groups_) out.groups.push_back({g.first, g.second});
  std::sort(out.groups.begin(), out.groups.end(),
            [](const std::pair<std::string, int>& a, const std::pair<std::string, int>& b) { return a.second < b.second; });
  out.walls.resize(nwalls_);
}

void DemEngine::restart_release()
{
  for (int k = 0; k < 3; k++) {
    if (rst_buf_[k]) (void)hipFree(rst_buf_[k]);
    rst_buf_[k] = nullptr;
    rst_cap_[k] = 0;
  }
}

// the blocks of restart_pack_device of one or more ranks, one after the other in host memory -> the columns of the file:
// atoms, their CSR ranges and the wall rows merged into ascending tag order (host data only; the writer thread's work)
void restart_blocks_to_data(const char* p, size_t nbytes, RestartData& d)
{
  struct Block {
    size_t n, nc, m[kMaxWalls];
    const int *I, *cp, *wt[kMaxWalls];
    const double *D, *cs, *ws[kMaxWalls];
    std::vector<size_t> off;
  };
  std::vector<Block> blocks;
  const size_t nwalls = d.walls.size();
  size_t pos = 0, N = 0, NC = 0;
  d.max_tag = 0;
  while (pos < nbytes) {
    long long hdr[16];
    if (pos + 128 > nbytes) fail("write_restart: a rank's block is cut short");
    memcpy(hdr, p + pos, 128);
    Block b;
    b.n = (size_t)hdr[0];
    b.nc = (size_t)hdr[1];
    d.max_tag = std::max(d.max_tag, hdr[2]);
    if ((size_t)hdr[3] != nwalls) fail("write_restart: the ranks disagree about the wall fixes");
    size_t msum = 0;
    for (size_t w = 0; w < nwalls; w++) msum += (b.m[w] = (size_t)hdr[4 + w]);
    const size_t nint = (5 * b.n + b.nc + msum + 1) & ~(size_t)1, ndbl = 20 * b.n + 3 * b.nc + 3 * msum;
    if (pos + 128 + 4 * nint + 8 * ndbl > nbytes) fail("write_restart: a rank's block is cut short");
    b.I = reinterpret_cast<const int*>(p + pos + 128);
    b.D = reinterpret_cast<const double*>(p + pos + 128 + 4 * nint);
    b.cp = b.I + 5 * b.n;
    b.cs = b.D + 20 * b.n;
    const int* wt = b.cp + b.nc;
    const double* ws = b.cs + 3 * b.nc;
    for (size_t w = 0; w < nwalls; w++) {
      b.wt[w] = wt;
      b.ws[w] = ws;
      wt += b.m[w];
      ws += 3 * b.m[w];
    }
    b.off.assign(b.n + 1, 0);
    for (size_t i = 0; i < b.n; i++) b.off[i + 1] = b.off[i] + (size_t)b.I[4 * b.n + i];
    if (b.off[b.n] != b.nc) fail("write_restart: a rank's contact counts do not sum to its contacts");
    N += b.n;
    NC += b.nc;
    pos += 128 + 4 * nint + 8 * ndbl;
    blocks.push_back(std::move(b));
  }
  struct Ref {
    int tag;
    unsigned blk;
    size_t idx;
  };
  auto by_tag = [](const Ref& a, const Ref& b) { return a.tag < b.tag; };
  std::vector<Ref> order;
  order.reserve(N);
  for (size_t k = 0; k < blocks.size(); k++)
    for (size_t i = 0; i < blocks[k].n; i++) order.push_back({blocks[k].I[i], (unsigned)k, i});
  if (blocks.size() > 1) std::sort(order.begin(), order.end(), by_tag);   // (one block is in tag order already)
  d.natoms = (long long)N;
  d.ncontacts = (long long)NC;
  d.tag.resize(N); d.type.resize(N); d.mask.resize(N); d.foam.resize(N); d.ccount.resize(N);
  d.x.resize(3 * N); d.radius.resize(N); d.v.resize(3 * N); d.rmass.resize(N); d.omega.resize(3 * N);
  d.fdrag.resize(3 * N); d.DuDt.resize(3 * N); d.vOld.resize(3 * N);
  d.cpartner.resize(NC); d.cshear.resize(3 * NC);
  size_t e = 0;
  for (size_t r = 0; r < N; r++) {
    const Block& b = blocks[order[r].blk];
    const size_t i = order[r].idx, n = b.n;
    d.tag[r] = b.I[i]; d.type[r] = b.I[n + i]; d.mask[r] = b.I[2 * n + i]; d.foam[r] = b.I[3 * n + i];
    d.ccount[r] = b.I[4 * n + i];
    d.radius[r] = b.D[3 * n + i];
    d.rmass[r] = b.D[7 * n + i];
    for (size_t c = 0; c < 3; c++) {
      d.x[c * N + r] = b.D[c * n + i];
      d.v[c * N + r] = b.D[4 * n + c * n + i];
      d.omega[c * N + r] = b.D[8 * n + c * n + i];
      d.fdrag[c * N + r] = b.D[11 * n + c * n + i];
      d.DuDt[c * N + r] = b.D[14 * n + c * n + i];
      d.vOld[c * N + r] = b.D[17 * n + c * n + i];
    }
    for (size_t k = b.off[i]; k < b.off[i + 1]; k++, e++) {
      d.cpartner[e] = b.cp[k];
      for (size_t c = 0; c < 3; c++) d.cshear[c * NC + e] = b.cs[c * b.nc + k];
    }
  }
  for (size_t w = 0; w < nwalls; w++) {
    std::vector<Ref> rows;
    for (size_t k = 0; k < blocks.size(); k++)
      for (size_t i = 0; i < blocks[k].m[w]; i++) rows.push_back({blocks[k].wt[w][i], (unsigned)k, i});
    if (blocks.size() > 1) std::sort(rows.begin(), rows.end(), by_tag);
    const size_t m = rows.size();
    d.walls[w].tag.resize(m);
    d.walls[w].shear.resize(3 * m);
    for (size_t r = 0; r < m; r++) {
      const Block& b = blocks[rows[r].blk];
      d.walls[w].tag[r] = rows[r].tag;
      for (size_t c = 0; c < 3; c++) d.walls[w].shear[c * m + r] = b.ws[w][c * b.m[w] + rows[r].idx];
    }
  }
}

void DemEngine::restart_unpack(const RestartData& in, const std::vector<int>& keep)
{
  if (nlocal_ || setup_done_) fail("read_restart: the engine already holds atoms");
  const int N = (int)in.natoms, nkeep = (int)keep.size(), nc = (int)in.ncontacts;
  max_tag_ = std::max(max_tag_, (int)in.max_tag);
  dt_ = in.dt;
  nlocal_ = 0;
  if (!nkeep) return;
  ensure_capacity((size_t)nkeep + (size_t)nkeep / 2 + 4096);
  const size_t n = (size_t)N;
  DevBuf bi(sizeof(int) * 4 * n), bd(sizeof(double) * 20 * n), bkeep(sizeof(int) * (size_t)nkeep);
  auto upi = [&](int* dst, const std::vector<int>& v) {
    if (!v.empty()) SF_HIP(hipMemcpyAsync(dst, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice, stream_));
  };
  auto upd = [&](double* dst, const std::vector<double>& v) {
    if (!v.empty()) SF_HIP(hipMemcpyAsync(dst, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, stream_));
  };
  int* I = bi.as<int>();
  double* D = bd.as<double>();
  RstFileCols F;
  F.tag = I; F.type = I + n; F.mask = I + 2 * n; F.foam = I + 3 * n;
  F.x = D; F.radius = D + 3 * n; F.v = D + 4 * n; F.rmass = D + 7 * n; F.omega = D + 8 * n; F.fdrag = D + 11 * n;
  F.DuDt = D + 14 * n; F.vOld = D + 17 * n;
  upi(I, in.tag); upi(I + n, in.type); upi(I + 2 * n, in.mask); upi(I + 3 * n, in.foam);
  upd(D, in.x); upd(D + 3 * n, in.radius); upd(D + 4 * n, in.v); upd(D + 7 * n, in.rmass); upd(D + 8 * n, in.omega);
  upd(D + 11 * n, in.fdrag); upd(D + 14 * n, in.DuDt); upd(D + 17 * n, in.vOld);
  up(bkeep, keep, stream_);
  for (int k : keep) rmax_ = std::max(rmax_, in.radius[(size_t)k]);
  // (every wall row starts clear: the rows a fix claims are written by restart_wall_rows)
  SF_HIP(hipMemsetAsync(wshear_.ptr, 0, sizeof(double) * 3 * kMaxWalls * cap_, stream_));
  k_rst_unpack_atoms<<<div_up(nkeep, 256), 256, 0, stream_>>>(
      bkeep.as<int>(), nkeep, N, F, 0, xr_[cur_].as<double4>(), vm_[cur_].as<double4>(), om_[cur_].as<double4>(), tag_.as<int>(),
      type_.as<int>(), mask_.as<int>(), foamCpuId_.as<int>(), fdrag_.as<double>(), DuDt_.as<double>(), vOld_.as<double>(),
      numneigh_.as<int>(), wtouch_.as<unsigned char>(), cap_);
  restart_launches_++;
  for (int r = 0; r < nextra_; r++)   // client rows are not in the file: their initial value, as for created atoms
    if (extra_used_ & (1u << r)) {
      std::vector<double> row((size_t)nkeep, extra_init_[r]);
      SF_HIP(hipMemcpyAsync(extra_.as<double>() + (size_t)r * cap_, row.data(), sizeof(double) * nkeep, hipMemcpyHostToDevice,
                            stream_));
      sync();
    }
  int longest = 0;
  if (nc) {
    // CSR offsets and the file position -> local index table (host data, one pass each)
    std::vector<int> off(n + 1, 0), loc(n, -1);
    for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + in.ccount[i];
    for (int k = 0; k < nkeep; k++) loc[(size_t)keep[k]] = k;
    DevBuf boff(sizeof(int) * (n + 1)), bloc(sizeof(int) * n), bcp(sizeof(int) * (size_t)nc), bcs(sizeof(double) * 3 * (size_t)nc);
    up(boff, off, stream_);
    up(bloc, loc, stream_);
    up(bcp, in.cpartner, stream_);
    up(bcs, in.cshear, stream_);
    hist_buf_ = cur_ ^ 1;
    auto expand = [&](int fill) {
      k_rst_expand<<<div_up(nc, 256), 256, 0, stream_>>>(nc, N, boff.as<int>(), F.tag, bcp.as<int>(), bcs.as<double>(),
                                                         bloc.as<int>(), 0, fill, M_, numneigh_.as<int>(), ptag_.as<int>(),
                                                         shear_[hist_buf_].as<double>(), cap_);
      restart_launches_++;
    };
    expand(0);   // (row lengths first: the slot-major arrays may have to grow)
    std::vector<int> deg((size_t)nkeep);
    SF_HIP(hipMemcpyAsync(deg.data(), numneigh_.ptr, sizeof(int) * nkeep, hipMemcpyDeviceToHost, stream_));
    sync();
    for (int d : deg) longest = std::max(longest, d);
    if (longest > M_) grow_neigh(longest + 4);
    SF_HIP(hipMemsetAsync(numneigh_.ptr, 0, sizeof(int) * nkeep, stream_));
    expand(1);
  }
  sync();
  nlocal_ = nkeep;
  order_version_++;
  restart_order_ = order_version_;
  if (longest > 0) {
    max_neigh_used_ = std::max(max_neigh_used_, longest);
    mrec_ = std::max(mrec_, longest);
    hist_rows_ = true;
  }
}

void DemEngine::restart_wall_rows(int w, const std::vector<int>& tag, const std::vector<double>& shear3)
{
  if (w < 0 || w >= nwalls_) fail("no such wall fix %d", w);
  const size_t m = tag.size();
  if (!m || !nlocal_) return;
  if (restart_order_ != order_version_ || setup_done_)
    fail("the wall rows of a restart file can only be restored before the first run");
  DevBuf bt(sizeof(int) * m), bs(sizeof(double) * 3 * m);
  up(bt, tag, stream_);
  up(bs, shear3, stream_);
  k_rst_wall_rows<<<div_up((long long)m, 256), 256, 0, stream_>>>(bt.as<int>(), bs.as<double>(), (int)m, tag_.as<int>(), nlocal_,
                                                                 w, wshear_.as<double>(), wtouch_.as<unsigned char>(), cap_);
  restart_launches_++;
  sync();
}

// ------------------------------------------------------------------------------------------------
// script surface
// ------------------------------------------------------------------------------------------------
namespace {

// One checkpoint on its way to the disk: the blocks in pinned memory (the copy is ordered behind the pack by an event and
// runs on a side stream), the header fields, the file name.  The writer thread waits for the copy, merges the blocks
// into the file's columns, computes the checksums, writes FILE.tmp, flushes and renames -- the sub-steps queued behind
// the pack do not wait for any of it.
struct Restart {
  std::vector<std::string> wall_ids;        // fix ID of engine wall w
  std::vector<RestartWall> pending;         // rows of a restart file no fix has claimed yet
  long long every = 0;                      // restart N ...
  std::string names[2];
  int nnames = 0, toggle = 0;
  long long last_written = -1;
  // rank 0 of a decomposed run: every rank's block (dump_gather)
  char* gathered = nullptr;
  size_t gathered_cap = 0;
  // the writer
  char* host = nullptr;   // pinned
  size_t host_cap = 0;
  hipStream_t side = nullptr;
  hipEvent_t ev_pack = nullptr, ev_copy = nullptr;
  struct Job {
    std::string path;
    size_t nbytes = 0;
    RestartData meta;
  };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> q;
  bool stop = false;
  std::string error;   // the first write error, thrown at the next drain
  std::thread th;
  // what the last checkpoint cost (tools/restart_cost.py): GPU ms of the pack, host ms from the call until the copy has
  // landed in pinned memory and until the file was renamed, its bytes
  double t_pack_ms = 0.0, t_copy_ms = 0.0, t_file_ms = 0.0, file_bytes = 0.0;
  std::chrono::steady_clock::time_point t0;
  bool timing = false;

  Restart() { th = std::thread([this] { loop(); }); }
  ~Restart()
  {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;   // (the loop leaves only with an empty queue: the files are complete)
    }
    cv.notify_all();
    th.join();
    if (host) (void)hipHostFree(host);
    if (gathered) (void)hipFree(gathered);
    if (ev_pack) (void)hipEventDestroy(ev_pack);
    if (ev_copy) (void)hipEventDestroy(ev_copy);
    if (side) (void)hipStreamDestroy(side);
  }
  void loop()
  {
    for (;;) {
      Job* j;
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [this] { return stop || !q.empty(); });
        if (q.empty()) return;
        j = &q.front();
      }
      std::string err;
      try {
        if (hipEventSynchronize(ev_copy) != hipSuccess) fail("restart: the copy of a checkpoint failed");
        const auto t1 = std::chrono::steady_clock::now();
        restart_blocks_to_data(host, j->nbytes, j->meta);
        restart_file_write(j->path, j->meta);
        const auto t2 = std::chrono::steady_clock::now();
        t_copy_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t_file_ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
      } catch (const std::exception& ex) {
        err = ex.what();
      }
      {
        std::lock_guard<std::mutex> g(mu);
        q.pop_front();
        if (!err.empty() && error.empty()) error = err;
      }
      cv.notify_all();
    }
  }
  void drain()
  {
    std::string e;
    {
      std::unique_lock<std::mutex> g(mu);
      cv.wait(g, [this] { return q.empty(); });
      e.swap(error);
    }
    if (!e.empty()) fail("%s", e.c_str());
  }
};

Restart& ensure(SfLammps& L) { return L.restart.ensure<Restart>(); }
const Restart* peek(const SfLammps& L) { return L.restart.get<Restart>(); }

std::string with_step(const std::string& name, long long step)
{
  const size_t star = name.find('*');
  if (star == std::string::npos) return name;
  return name.substr(0, star) + std::to_string(step) + name.substr(star + 1);
}

void refuse_percent(const std::string& name)
{
  if (name.find('%') != std::string::npos)
    fail("restart file name %s: the %% form (one file per rank) is not supported, a checkpoint is one file", name.c_str());
}

// pack on the engine's stream, gather on a decomposed run, then hand the blocks to the writer (rank 0); returns without
// waiting for the disk
void write_begin(SfLammps& L, const std::string& file)
{
  Restart& R = ensure(L);
  R.drain();   // (a checkpoint that comes due while the previous one is being written waits for it; its error surfaces here)
  R.t0 = std::chrono::steady_clock::now();
  DemEngine& e = L.eng;
  hipStream_t s = e.stream();
  const char* blob = nullptr;
  size_t nbytes = e.restart_pack_device(&blob, R.timing ? &R.t_pack_ms : nullptr);
  if (L.decomposed || L.world_size > 1) {
    unsigned long long atoms = 0;
    nbytes = dump_gather(L, blob, nbytes, (unsigned long long)e.nlocal(), &R.gathered, &R.gathered_cap, &atoms);
    if (L.world_rank != 0) return;   // (only rank 0 creates a file)
    blob = R.gathered;
  }
  if (nbytes > R.host_cap) {
    if (R.host) SF_HIP(hipHostFree(R.host));
    R.host_cap = nbytes + nbytes / 4 + 4096;
    SF_HIP(hipHostMalloc(reinterpret_cast<void**>(&R.host), R.host_cap));
  }
  if (!R.side) {
    SF_HIP(hipStreamCreateWithFlags(&R.side, hipStreamNonBlocking));
    SF_HIP(hipEventCreateWithFlags(&R.ev_pack, hipEventDisableTiming));
    SF_HIP(hipEventCreateWithFlags(&R.ev_copy, hipEventDisableTiming));
  }
  SF_HIP(hipEventRecord(R.ev_pack, s));
  SF_HIP(hipStreamWaitEvent(R.side, R.ev_pack, 0));
  SF_HIP(hipMemcpyAsync(R.host, blob, nbytes, hipMemcpyDeviceToHost, R.side));
  SF_HIP(hipEventRecord(R.ev_copy, R.side));
  Restart::Job j;
  j.path = file;
  j.nbytes = nbytes;
  e.restart_describe(j.meta);
  j.meta.units_lj = thermo_units_lj(L) ? 1 : 0;
  for (size_t w = 0; w < j.meta.walls.size(); w++)
    j.meta.walls[w].id = w < R.wall_ids.size() ? R.wall_ids[w] : ("wall" + std::to_string(w));
  {
    std::lock_guard<std::mutex> g(R.mu);
    R.q.push_back(std::move(j));
  }
  R.cv.notify_all();
}

}  // namespace

void restart_drain(SfLammps& L)
{
  if (L.restart) L.restart.get<Restart>()->drain();
}

void write_restart_command(SfLammps& L, const std::string& file)
{
  if (!L.eng.box_defined()) fail("Write_restart command before simulation box is defined");
  refuse_percent(file);
  write_begin(L, with_step(file, L.eng.nsteps()));
  restart_drain(L);   // (returns when the file is complete)
}

void restart_timing(SfLammps& L, bool on) { ensure(L).timing = on; }

void restart_last_cost(SfLammps& L, double out[4])
{
  Restart& R = ensure(L);
  R.drain();
  out[0] = R.t_pack_ms;
  out[1] = R.t_copy_ms;
  out[2] = R.t_file_ms;
  out[3] = 0.0;
}

void restart_command(SfLammps& L, const std::vector<std::string>& w)
{
  if (w.size() < 2) fail("Illegal restart command");
  char* end = nullptr;
  const long long n = std::strtoll(w[1].c_str(), &end, 10);
  if (end == w[1].c_str() || *end != '\0' || n < 0) fail("Illegal restart command");
  Restart& R = ensure(L);
  if (n == 0) {
    if (w.size() != 2) fail("Illegal restart command");
    R.every = 0;
    R.nnames = 0;
    return;
  }
  if (w.size() != 3 && w.size() != 4) fail("Illegal restart command");
  for (size_t k = 2; k < w.size(); k++) refuse_percent(w[k]);
  R.every = n;
  R.nnames = (int)w.size() - 2;
  R.names[0] = w[2];
  R.names[1] = R.nnames == 2 ? w[3] : "";
  if (R.nnames == 1 && R.names[0].find('*') == std::string::npos) R.names[0] += ".*";   // ROOT -> ROOT.<step>
  R.toggle = 1;   // (the first checkpoint goes to FILE2: after an even number of them the newest one is FILE1)
  R.last_written = L.eng.nsteps();   // ([3P] Output: the next checkpoint is the next multiple of N after the current step)
}

void restart_set_pending_walls(SfLammps& L, std::vector<RestartWall>&& walls) { ensure(L).pending = std::move(walls); }

void restart_fix_wall(SfLammps& L, const std::string& id, int w)
{
  Restart& R = ensure(L);
  if ((int)R.wall_ids.size() <= w) R.wall_ids.resize(w + 1);
  R.wall_ids[w] = id;
  for (size_t k = 0; k < R.pending.size(); k++)
    if (R.pending[k].id == id) {
      L.eng.restart_wall_rows(w, R.pending[k].tag, R.pending[k].shear);
      R.pending.erase(R.pending.begin() + k);
      break;
    }
}

bool restart_active(const SfLammps& L)
{
  const Restart* R = peek(L);
  return R && R->every > 0;
}

void restart_run_begin(SfLammps& L)
{
  Restart* R = L.restart.get<Restart>();
  if (!R || R->pending.empty()) return;
  for (const RestartWall& w : R->pending) {
    const std::string msg = "WARNING: restart file: the saved state of fix " + w.id + " (" + std::to_string(w.tag.size()) +
                            " wall contacts) was not claimed by a fix of that ID and is dropped";
    thermo_echo(L, msg);
    if (L.world_rank == 0) fprintf(stderr, "%s\n", msg.c_str());
  }
  R->pending.clear();
}

long long restart_next_step(const SfLammps& L, long long step)
{
  const Restart* R = peek(L);
  if (!R || R->every <= 0) return -1;
  return (step / R->every + 1) * R->every;
}

void restart_write_due(SfLammps& L)
{
  Restart* R = L.restart.get<Restart>();
  if (!R || R->every <= 0) return;
  const long long step = L.eng.nsteps();
  if (step % R->every != 0 || step == R->last_written) return;
  const std::string& name = R->names[R->nnames == 2 ? R->toggle : 0];
  if (R->nnames == 2) R->toggle ^= 1;
  R->last_written = step;
  write_begin(L, with_step(name, step));
}

long long restart_launches(const SfLammps& L) { return L.eng.restart_launches(); }

}  // namespace sf
