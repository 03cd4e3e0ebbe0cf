// sf_chunk_parse.h -- the words of `compute ID group chunk/atom bin/1d|2d|3d ...` and `fix ID group ave/chunk ...`, the
// bins they define and the sample schedule ([3P] LAMMPS names and rules: ComputeChunkAtom::setup_xyz_bins / atom2bin*,
// FixAveChunk::FixAveChunk / nextvalid), on the host with nothing but the standard library, so that this code can be
// compiled into a stand-alone program and run under the host sanitizers (sf_compute_parse.h is the precedent).  Every
// parser returns an empty string, or the error text.  The schedule, the file keywords and the c_ID[k] parser are those of
// sf_ave_common.h; split_quoted, chunk_parse_double and ave_format_ok are here for the other parse headers.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sf_ave_common.h"

namespace sf {

// the words of a line, with "..." and '...' kept together (the title keywords carry spaces); `#` outside quotes ends it
inline std::string split_quoted(const std::string& line, std::vector<std::string>* w)
{
  w->clear();
  size_t k = 0;
  const size_t n = line.size();
  while (k < n) {
    while (k < n && (line[k] == ' ' || line[k] == '\t' || line[k] == '\r' || line[k] == '\n')) k++;
    if (k >= n || line[k] == '#') break;
    std::string t;
    if (line[k] == '"' || line[k] == '\'') {
      const char q = line[k++];
      const size_t e = line.find(q, k);
      if (e == std::string::npos) return "Unbalanced quotes in input line";
      t = line.substr(k, e - k);
      k = e + 1;
    } else {
      while (k < n && line[k] != ' ' && line[k] != '\t' && line[k] != '\r' && line[k] != '\n') t += line[k++];
    }
    w->push_back(t);
  }
  return std::string();
}

inline bool chunk_parse_double(const std::string& s, double* v)
{
  if (s.empty()) return false;
  char* end = nullptr;
  *v = std::strtod(s.c_str(), &end);
  return end != s.c_str() && *end == '\0' && *v == *v && *v - *v == 0.0;   // (a finite number, all of the word)
}

// The bins of a chunk/atom compute, per binned dimension k (the first one named varies slowest in the chunk ID); plain
// data: the assign kernel takes it by value
constexpr int kChunkMax = 1 << 24;
struct ChunkBins {
  int ndim = 0;
  int nchunk = 0;
  int dim[3] = {0, 0, 0};         // 0 1 2 = x y z
  int nlayers[3] = {1, 1, 1};
  int discard[3] = {0, 0, 0};     // 1: an atom outside the layers of this dimension gets chunk ID 0;  0: the end layer
  int periodic[3] = {0, 0, 0};    // remap into [boxlo, boxhi) first
  double offset[3] = {0, 0, 0}, delta[3] = {1, 1, 1}, invdelta[3] = {1, 1, 1};
  double boxlo[3] = {0, 0, 0}, boxhi[3] = {1, 1, 1}, prd[3] = {1, 1, 1};
  double volume = 1.0;            // of one chunk: the deltas of the binned dimensions x the box lengths of the others
};

// one dimension's layers from origin, delta and the extent [minvalue, maxvalue] they must cover
inline void chunk_layers(double origin, double delta, double minvalue, double maxvalue, double* offset, double* invdelta_out,
                         long long* nlayers)
{
  const double invdelta = 1.0 / delta;
  double lo = origin + (double)(long long)((minvalue - origin) * invdelta) * delta;
  if (lo > minvalue) lo -= delta;
  double hi = origin + (double)(long long)((maxvalue - origin) * invdelta) * delta;
  if (hi < maxvalue) hi += delta;
  *offset = lo;
  *invdelta_out = invdelta;
  *nlayers = (long long)((hi - lo) * invdelta + 0.5);
}

// w = compute ID group chunk/atom STYLE ...; boxlo / boxhi / periodic: the box as it stands (reduced units and the words
// lower / center / upper are converted here, at the definition)
inline std::string parse_chunk_atom(const std::vector<std::string>& w, const double boxlo[3], const double boxhi[3],
                                    const int periodic[3], ChunkBins* out)
{
  const std::string illegal = "Illegal compute chunk/atom command";
  if (w.size() < 5) return illegal;
  const std::string& style = w[4];
  int ndim = 0;
  if (style == "bin/1d") ndim = 1;
  else if (style == "bin/2d") ndim = 2;
  else if (style == "bin/3d") ndim = 3;
  else if (style == "type" || style == "molecule" || style == "bin/sphere" || style == "bin/cylinder" ||
           style.compare(0, 2, "c_") == 0 || style.compare(0, 2, "f_") == 0 || style.compare(0, 2, "v_") == 0)
    return "compute chunk/atom: style " + style + " is not supported (bin/1d, bin/2d and bin/3d are)";
  else
    return illegal;
  enum { LOWER, CENTER, UPPER, COORD };
  auto dim_of = [](const std::string& s) { return s == "x" ? 0 : (s == "y" ? 1 : (s == "z" ? 2 : -1)); };
  int dim[3] = {0, 0, 0}, oflag[3] = {0, 0, 0};
  double origin[3] = {0, 0, 0}, delta[3] = {0, 0, 0};
  size_t k = 5;
  if (w.size() < k + 3 * (size_t)ndim) return illegal;
  for (int a = 0; a < ndim; a++, k += 3) {
    dim[a] = dim_of(w[k]);
    if (dim[a] < 0) return illegal;
    for (int b = 0; b < a; b++)
      if (dim[b] == dim[a]) return illegal;
    if (w[k + 1] == "lower") oflag[a] = LOWER;
    else if (w[k + 1] == "center") oflag[a] = CENTER;
    else if (w[k + 1] == "upper") oflag[a] = UPPER;
    else {
      oflag[a] = COORD;
      if (!chunk_parse_double(w[k + 1], &origin[a])) return illegal;
    }
    if (!chunk_parse_double(w[k + 2], &delta[a]) || !(delta[a] > 0.0)) return illegal;
  }
  // keywords
  int units = -1;                      // 0 box, 1 reduced
  int discard = 2;                     // 0 no, 1 yes, 2 mixed
  bool has_bound[3] = {false, false, false};   // by box dimension
  int minflag[3] = {LOWER, LOWER, LOWER}, maxflag[3] = {UPPER, UPPER, UPPER};
  double minv[3] = {0, 0, 0}, maxv[3] = {0, 0, 0};
  while (k < w.size()) {
    const std::string& key = w[k];
    const size_t left = w.size() - k - 1;
    if (key == "units") {
      if (left < 1) return illegal;
      if (w[k + 1] == "box") units = 0;
      else if (w[k + 1] == "reduced") units = 1;
      else if (w[k + 1] == "lattice")
        return "compute chunk/atom: units lattice is not supported (there is no lattice command): give units box or reduced";
      else return illegal;
      k += 2;
    } else if (key == "bound") {
      if (left < 3) return illegal;
      const int d = dim_of(w[k + 1]);
      if (d < 0) return illegal;
      has_bound[d] = true;
      if (w[k + 2] == "lower") minflag[d] = LOWER;
      else {
        minflag[d] = COORD;
        if (!chunk_parse_double(w[k + 2], &minv[d])) return illegal;
      }
      if (w[k + 3] == "upper") maxflag[d] = UPPER;
      else {
        maxflag[d] = COORD;
        if (!chunk_parse_double(w[k + 3], &maxv[d])) return illegal;
      }
      k += 4;
    } else if (key == "discard") {
      if (left < 1) return illegal;
      if (w[k + 1] == "no") discard = 0;
      else if (w[k + 1] == "yes") discard = 1;
      else if (w[k + 1] == "mixed") discard = 2;
      else return illegal;
      k += 2;
    } else if (key == "nchunk") {
      if (left < 1 || (w[k + 1] != "once" && w[k + 1] != "every")) return illegal;
      k += 2;   // (the bins are those of the definition either way: the box does not change)
    } else if (key == "ids") {
      if (left < 1) return illegal;
      if (w[k + 1] == "once" || w[k + 1] == "nfreq")
        return "compute chunk/atom: ids " + w[k + 1] + " is not supported (ids every is: an atom is assigned anew at every sample)";
      if (w[k + 1] != "every") return illegal;
      k += 2;
    } else if (key == "limit") {
      long v = 0;
      if (left < 1 || !chunk_parse_int(w[k + 1], &v) || v < 0) return illegal;
      if (v > 0) return "compute chunk/atom: limit " + w[k + 1] + " is not supported (limit 0 is)";
      k += 2;
    } else if (key == "compress") {
      if (left < 1) return illegal;
      if (w[k + 1] == "yes") return "compute chunk/atom: compress yes is not supported (compress no is)";
      if (w[k + 1] != "no") return illegal;
      k += 2;
    } else if (key == "pbc") {
      if (left < 1) return illegal;
      if (w[k + 1] == "yes") return "compute chunk/atom: pbc yes is not supported (pbc no is)";
      if (w[k + 1] != "no") return illegal;
      k += 2;
    } else if (key == "region") {
      return "compute chunk/atom: region is not supported (give the compute a region group: group ID region RID, or group ID dynamic)";
    } else
      return illegal;
  }
  if (units < 0)
    return "compute chunk/atom: give units box (or reduced): LAMMPS' default is units lattice, and there is no lattice command";
  ChunkBins B;
  B.ndim = ndim;
  B.volume = 1.0;
  bool binned[3] = {false, false, false};
  long long nchunk = 1;
  for (int a = 0; a < ndim; a++) {
    const int d = dim[a];
    binned[d] = true;
    const double lo = boxlo[d], hi = boxhi[d], prd = hi - lo;
    if (!(prd > 0.0)) return "compute chunk/atom: the box is not defined yet";
    double del = delta[a], org = origin[a], mn = minv[d], mx = maxv[d];
    if (units == 1) {   // fractions of the box length
      del *= prd;
      org = lo + org * prd;
      mn = lo + mn * prd;
      mx = lo + mx * prd;
    }
    if (oflag[a] == LOWER) org = lo;
    else if (oflag[a] == UPPER) org = hi;
    else if (oflag[a] == CENTER) org = 0.5 * (lo + hi);
    const double minvalue = minflag[d] == COORD ? mn : lo, maxvalue = maxflag[d] == COORD ? mx : hi;
    if (!(minvalue < maxvalue)) return illegal;
    if (!(del > 0.0) || (maxvalue - minvalue) / del > (double)kChunkMax) return "compute chunk/atom: too many layers";
    long long nl = 0;
    chunk_layers(org, del, minvalue, maxvalue, &B.offset[a], &B.invdelta[a], &nl);
    if (nl < 1) return illegal;
    nchunk *= nl;
    if (nchunk > kChunkMax) return "compute chunk/atom: more than 16777216 chunks";
    B.dim[a] = d;
    B.nlayers[a] = (int)nl;
    B.delta[a] = del;
    B.discard[a] = discard == 1 || (discard == 2 && has_bound[d]) ? 1 : 0;
    B.periodic[a] = periodic[d] ? 1 : 0;
    B.boxlo[a] = lo;
    B.boxhi[a] = hi;
    B.prd[a] = prd;
    B.volume *= del;
  }
  for (int d = 0; d < 3; d++)
    if (!binned[d]) B.volume *= boxhi[d] - boxlo[d];
  B.nchunk = (int)nchunk;
  *out = B;
  return std::string();
}

// the layer of coordinate x in binned dimension a, or -1 (discarded); the kernel evaluates the same expressions
inline int chunk_layer_of(const ChunkBins& B, int a, double x)
{
  double xr = x;
  if (B.periodic[a]) {
    if (xr < B.boxlo[a]) xr += B.prd[a];
    if (xr >= B.boxhi[a]) xr -= B.prd[a];
  }
  int ibin = (int)((xr - B.offset[a]) * B.invdelta[a]);
  if (xr < B.offset[a]) ibin--;
  if (ibin < 0) return B.discard[a] ? -1 : 0;
  if (ibin > B.nlayers[a] - 1) return B.discard[a] ? -1 : B.nlayers[a] - 1;
  return ibin;
}

// ---- fix ave/chunk ----

enum AveSource { AS_VX, AS_VY, AS_VZ, AS_FX, AS_FY, AS_FZ, AS_DENSITY_NUMBER, AS_DENSITY_MASS, AS_COMPUTE };
constexpr int kAveMaxValues = 24;

struct AveValue {
  int source = AS_VX;
  std::string word;   // as typed (the file's header line)
  std::string id;     // AS_COMPUTE
  long index = 0;     // AS_COMPUTE: k of c_ID[k], 0: none
};

struct AveSpec : AveSchedule, AveFileSpec {
  std::string id, group, chunk;
  std::vector<AveValue> values;
  int norm = 0;          // 0 all, 1 sample, 2 none
  bool running = false;
  std::string format;    // empty: %g
};

// one conversion of a double and nothing else: % [flags] [width] [.precision] e|E|f|F|g|G
inline bool ave_format_ok(const std::string& f)
{
  size_t k = 0;
  if (f.size() < 2 || f.size() > 30 || f[k++] != '%') return false;
  while (k < f.size() && std::strchr("-+ #0", f[k])) k++;
  size_t digits = 0;
  while (k < f.size() && f[k] >= '0' && f[k] <= '9') k++, digits++;
  if (digits > 3) return false;
  if (k < f.size() && f[k] == '.') {
    k++;
    digits = 0;
    while (k < f.size() && f[k] >= '0' && f[k] <= '9') k++, digits++;
    if (digits > 3) return false;
  }
  return k + 1 == f.size() && std::strchr("eEfFgG", f[k]) != nullptr;
}

// w = fix ID group ave/chunk Nevery Nrepeat Nfreq chunkID value ... keywords (split_quoted words)
inline std::string parse_ave_chunk(const std::vector<std::string>& w, AveSpec* out)
{
  const std::string illegal = "Illegal fix ave/chunk command";
  if (w.size() < 9) return illegal;
  AveSpec S;
  S.id = w[1];
  S.group = w[2];
  if (!S.parse(w, 4, illegal).empty()) return illegal;
  S.chunk = w[7];
  static const char* const plain[8] = {"vx", "vy", "vz", "fx", "fy", "fz", "density/number", "density/mass"};
  size_t k = 8;
  for (; k < w.size(); k++) {
    const std::string& s = w[k];
    AveValue v;
    v.word = s;
    int src = -1;
    for (int q = 0; q < 8; q++)
      if (s == plain[q]) src = q;
    if (src >= 0) v.source = src;
    else if (s == "temp")
      return "fix ave/chunk: temp is not supported (Boltzmann's constant means nothing for grains): average a compute ke/atom "
             "through c_ID";
    else if (s.compare(0, 2, "f_") == 0 || s.compare(0, 2, "v_") == 0)
      return "fix ave/chunk: " + s + " is not supported (f_ and v_ values are not; c_ID of a per-atom compute is)";
    else if (s.compare(0, 2, "c_") == 0) {
      v.source = AS_COMPUTE;
      if (!parse_cref(s, &v.id, &v.index)) return illegal;
    } else
      break;
    if ((int)S.values.size() >= kAveMaxValues) return "fix ave/chunk: more than 24 values";
    S.values.push_back(v);
  }
  if (S.values.empty()) return illegal;
  while (k < w.size()) {
    const std::string& key = w[k];
    const size_t left = w.size() - k - 1;
    const AveKey fk = ave_file_keyword(w, &k, &S);
    if (fk == AK_ERROR) return illegal;
    if (fk == AK_CONSUMED) continue;
    if (key == "norm") {
      if (left < 1) return illegal;
      if (w[k + 1] == "all") S.norm = 0;
      else if (w[k + 1] == "sample") S.norm = 1;
      else if (w[k + 1] == "none") S.norm = 2;
      else return illegal;
      k += 2;
    } else if (key == "ave") {
      if (left < 1) return illegal;
      if (w[k + 1] == "one") S.running = false;
      else if (w[k + 1] == "running") S.running = true;
      else if (w[k + 1] == "window") return "fix ave/chunk: ave window is not supported (ave one and ave running are)";
      else return illegal;
      k += 2;
    } else if (key == "format") {
      if (left < 1) return illegal;
      if (!ave_format_ok(w[k + 1]))
        return "fix ave/chunk: format " + w[k + 1] + " is not one %g-class conversion of a double (such as %.10g)";
      S.format = w[k + 1];
      k += 2;
    } else if (key == "bias" || key == "adof" || key == "cdof") {
      return "fix ave/chunk: " + key + " is not supported (it belongs to temp, which is not)";
    } else
      return illegal;
  }
  *out = S;
  return std::string();
}

}  // namespace sf
