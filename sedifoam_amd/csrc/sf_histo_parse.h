// sf_histo_parse.h -- the words of `fix ID group ave/histo Nevery Nrepeat Nfreq lo hi Nbin value ... keywords`, the bins
// they define, the bin of one value and the averaging of the output blocks (the rules of DESIGN.md section 16, LAMMPS names
// and wording), on the host with nothing but the standard library, so that this code can be compiled into a stand-alone
// program and run under the host sanitizers (sf_global_parse.h is the precedent; sf_chunk_parse.h holds split_quoted and
// chunk_parse_double; the schedule, the file, ave and start keywords, the attribute words and parse_cref are those of
// sf_ave_common.h).  The parser returns an empty string, or the error text.  histo_bin is also what the kernel of sf_histo.hip calls: one expression on both sides.
#pragma once
#include <deque>
#include <string>
#include <vector>

#include "sf_global_parse.h"

#if defined(__HIPCC__)
#define SF_HISTO_HD __host__ __device__
#else
#define SF_HISTO_HD
#endif

namespace sf {

constexpr int kHistoMaxBins = 8192;   // Nbin: the kernel keeps a block's counters in LDS
constexpr int kHistoMaxValues = 16;   // the columns of one launch (kGCols of sf_global.hip)
enum HistoMode { HM_SCALAR, HM_VECTOR };
enum HistoKind { HK_NONE = -1, HK_GLOBAL, HK_PERATOM, HK_LOCAL };
enum HistoBeyond { HB_IGNORE, HB_END, HB_EXTRA };

struct HistoValue {
  int attr = AA_X;
  std::string word;   // as typed
  std::string id;     // AA_COMPUTE
  long index = 0;     // AA_COMPUTE: k of c_ID[k], 0: none
};

struct HistoSpec : AveSchedule, AveFileSpec {
  std::string id, group;
  double lo = 0.0, hi = 1.0;
  long nbin = 1;
  std::vector<HistoValue> values;
  int mode = HM_SCALAR;
  int kind = HK_NONE;   // as typed (HK_NONE: not given)
  int beyond = HB_IGNORE;
  int ave = AVE_ONE;
  long window = 0;
};

// the bins: plain data, the kernel takes it by value
struct HistoBins {
  double lo, hi, bininv;
  int nbin;     // Nbin as typed
  int nbins;    // Nbin, or Nbin + 2 under beyond extra
  int beyond;
};

inline HistoBins histo_bins(double lo, double hi, long nbin, int beyond)
{
  HistoBins B;
  B.lo = lo;
  B.hi = hi;
  const double binsize = (hi - lo) / (double)nbin;
  B.bininv = 1.0 / binsize;
  B.nbin = (int)nbin;
  B.nbins = (int)nbin + (beyond == HB_EXTRA ? 2 : 0);
  B.beyond = beyond;
  return B;
}

inline double histo_coord(const HistoBins& B, int i)
{
  const double binsize = (B.hi - B.lo) / (double)B.nbin;
  if (B.beyond != HB_EXTRA) return B.lo + (i + 0.5) * binsize;
  if (i == 0) return B.lo;
  if (i == B.nbins - 1) return B.hi;
  return B.lo + (i - 1 + 0.5) * binsize;
}

// the bin of v in [0, nbins - 1], whatever v is; -1: ignored (beyond ignore: the value counts as missing)
SF_HISTO_HD inline int histo_bin(const HistoBins& B, double v)
{
  int ibin;
  if (v < B.lo) {
    if (B.beyond == HB_IGNORE) return -1;
    ibin = 0;
  } else if (v > B.hi) {
    if (B.beyond == HB_IGNORE) return -1;
    ibin = B.nbins - 1;
  } else {
    const double s = (v - B.lo) * B.bininv;   // (in [0, Nbin] up to a rounding; a NaN gives bin 0)
    ibin = s == s ? (int)s : 0;
    ibin = ibin < B.nbins - 1 ? ibin : B.nbins - 1;
    if (B.beyond == HB_EXTRA) ibin++;
  }
  ibin = ibin < B.nbins - 1 ? ibin : B.nbins - 1;
  return ibin > 0 ? ibin : 0;
}

// w = fix ID group ave/histo Nevery Nrepeat Nfreq lo hi Nbin value ... keywords (split_quoted words)
inline std::string parse_ave_histo(const std::vector<std::string>& w, HistoSpec* out)
{
  const std::string illegal = "Illegal fix ave/histo command";
  if (w.size() > 3 && w[3] == "ave/histo/weight")
    return "fix ave/histo/weight is not supported (its weighted bins are floating-point sums: a deterministic version is the "
           "sort-and-segment path of fix ave/chunk, not the integer counters of fix ave/histo)";
  if (w.size() < 11) return illegal;
  HistoSpec S;
  S.id = w[1];
  S.group = w[2];
  if (!S.parse(w, 4, illegal).empty()) return illegal;
  if (!chunk_parse_double(w[7], &S.lo) || !chunk_parse_double(w[8], &S.hi) || !chunk_parse_int(w[9], &S.nbin)) return illegal;
  if (S.lo >= S.hi || S.nbin <= 0) return illegal;
  if (S.nbin > kHistoMaxBins)
    return "fix ave/histo: more than 8192 bins (a block of the binning kernel keeps its counters in LDS)";
  size_t k = 10;
  for (; k < w.size(); k++) {
    const std::string& s = w[k];
    HistoValue v;
    v.word = s;
    const int a = ave_attr_of(s);
    if (a >= 0) v.attr = a;
    else if (s.compare(0, 2, "f_") == 0 || s.compare(0, 2, "v_") == 0)
      return "fix ave/histo: " + s + " is not supported (f_ and v_ values are not; x y z vx vy vz fx fy fz, c_ID and c_ID[k] are)";
    else if (s.compare(0, 2, "c_") == 0) {
      v.attr = AA_COMPUTE;
      if (s.size() > 3 && s.compare(s.size() - 3, 3, "[*]") == 0)
        return "fix ave/histo: " + s + " is not supported (name the columns one by one: c_ID[1] c_ID[2] ...)";
      if (!parse_cref(s, &v.id, &v.index)) return illegal;
    } else
      break;
    if ((int)S.values.size() >= kHistoMaxValues) return "fix ave/histo: more than 16 values";
    S.values.push_back(v);
  }
  if (S.values.empty()) return illegal;
  while (k < w.size()) {
    const std::string& key = w[k];
    const size_t left = w.size() - k - 1;
    AveKey shared = ave_file_keyword(w, &k, &S);
    if (shared == AK_NOT_MINE) shared = ave_mode_keyword(w, &k, &S.ave, &S.window, &S.start);
    if (shared == AK_ERROR) return illegal;
    if (shared == AK_CONSUMED) continue;
    if (key == "mode") {
      if (left < 1) return illegal;
      if (w[k + 1] == "scalar") S.mode = HM_SCALAR;
      else if (w[k + 1] == "vector") S.mode = HM_VECTOR;
      else return illegal;
      k += 2;
    } else if (key == "kind") {
      if (left < 1) return illegal;
      if (w[k + 1] == "global") S.kind = HK_GLOBAL;
      else if (w[k + 1] == "peratom") S.kind = HK_PERATOM;
      else if (w[k + 1] == "local") S.kind = HK_LOCAL;
      else return illegal;
      k += 2;
    } else if (key == "beyond") {
      if (left < 1) return illegal;
      if (w[k + 1] == "ignore") S.beyond = HB_IGNORE;
      else if (w[k + 1] == "end") S.beyond = HB_END;
      else if (w[k + 1] == "extra") S.beyond = HB_EXTRA;
      else return illegal;
      k += 2;
    } else if (key == "append") {
      return "fix ave/histo: append is not supported (file is: the file is written anew)";
    } else
      return illegal;
  }
  *out = S;
  return std::string();
}

// ---- the output blocks ----

// one block: the counts of Nrepeat samples, and total, missing, min, max
struct HistoBlock {
  std::vector<double> count;
  double total = 0.0, missing = 0.0, min = 1.0e20, max = -1.0e20;
};

// ave one | running | window M over the blocks as they come (counts are whole numbers below 2^53: the sums are exact)
struct HistoAverager {
  int ave = AVE_ONE;
  long window = 0;
  HistoBlock run;                  // running: the sum of all blocks
  std::deque<HistoBlock> blocks;   // window: the last M blocks
  HistoBlock add(const HistoBlock& b)
  {
    if (ave == AVE_ONE) return b;
    if (ave == AVE_RUNNING) {
      if (run.count.empty()) run.count.assign(b.count.size(), 0.0);
      fold(&run, b);
      return run;
    }
    blocks.push_back(b);
    if ((long)blocks.size() > window) blocks.pop_front();
    HistoBlock s;
    s.count.assign(b.count.size(), 0.0);
    for (const HistoBlock& q : blocks) fold(&s, q);   // (oldest first)
    return s;
  }
  static void fold(HistoBlock* s, const HistoBlock& b)
  {
    for (size_t i = 0; i < b.count.size() && i < s->count.size(); i++) s->count[i] += b.count[i];
    s->total += b.total;
    s->missing += b.missing;
    s->min = b.min < s->min ? b.min : s->min;
    s->max = b.max > s->max ? b.max : s->max;
  }
};

}  // namespace sf
