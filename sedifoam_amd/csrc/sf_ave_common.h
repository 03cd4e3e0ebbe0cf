// sf_ave_common.h -- what fix ave/chunk, fix ave/time and fix ave/histo share that is not their reduction ([3P] LAMMPS
// names and rules: FixAveTime::FixAveTime / options / nextvalid and their twins in FixAveChunk and FixAveHisto; DESIGN.md
// section 14, "The schedule"): the sample schedule `Nevery Nrepeat Nfreq [start N]`, the keywords `file`, `overwrite`,
// `title1..3`, `ave one|running|window M` and `start`, the output file, the attribute words x .. fz and the one parser of a
// `c_ID` / `c_ID[k]` word.  Host only, with nothing but the standard library, so that this code can be compiled into a
// stand-alone program and run under the host sanitizers (tests/c_abi/ave_common_check.cpp).  A function that can refuse
// returns an empty string, or the error text.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <unistd.h>

namespace sf {

inline bool chunk_parse_int(const std::string& s, long* v)
{
  if (s.empty()) return false;
  char* end = nullptr;
  *v = std::strtol(s.c_str(), &end, 10);
  return end != s.c_str() && *end == '\0' && *v > -2000000000L && *v < 2000000000L;
}

// `word` = c_ID or c_ID[k]: the ID and k in 1 .. 1000000 (0: no index given).  k is digits and nothing else -- no sign, no
// blank -- and nothing follows the `]`, as in LAMMPS.  false: malformed; the caller has its own text for that
inline bool parse_cref(const std::string& word, std::string* id, long* index)
{
  if (word.size() < 3 || word.compare(0, 2, "c_") != 0) return false;
  *id = word.substr(2);
  *index = 0;
  const size_t br = id->find('[');
  if (br != std::string::npos) {
    const std::string digits = id->substr(br + 1, id->size() - br - 2);
    if (id->back() != ']' || digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos) return false;
    if (!chunk_parse_int(digits, index) || *index < 1 || *index > 1000000) return false;
    id->resize(br);
  }
  return !id->empty() && id->find(']') == std::string::npos;
}

// the per-atom attributes that compute reduce and fix ave/histo take by name, and a compute behind c_ID
enum AveAttr { AA_X, AA_Y, AA_Z, AA_VX, AA_VY, AA_VZ, AA_FX, AA_FY, AA_FZ, AA_COMPUTE };

// AA_X .. AA_FZ, or -1
inline int ave_attr_of(const std::string& word)
{
  static const char* const names[9] = {"x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"};
  for (int q = 0; q < 9; q++)
    if (word == names[q]) return q;
  return -1;
}

// ---- the schedule ----

// the first step >= t0 at which a fix defined at step t0 samples ([3P] FixAveChunk::nextvalid; with `start`, the keyword of
// fix ave/time and ave/histo, [3P] FixAveTime::nextvalid: no output before step `start`)
inline long long ave_first_valid(long long t0, long long nevery, long long nrepeat, long long nfreq, long long start = 0)
{
  long long nv = (t0 / nfreq) * nfreq + nfreq;
  while (nv < start) nv += nfreq;
  if (nv - nfreq == t0 && nrepeat == 1) nv = t0;
  else nv -= (nrepeat - 1) * nevery;
  if (nv < t0) nv += nfreq;
  return nv;
}

// Nrepeat samples, Nevery steps apart, end at every multiple of Nfreq, where their average is put out
struct AveSchedule {
  long nevery = 1, nrepeat = 1, nfreq = 1;
  long start = 0;          // no output before this step (fix ave/chunk has no such keyword: 0)
  long long nvalid = 0;    // the next sample step
  int irepeat = 0;         // samples taken of the output under way

  // the three words w[k], w[k + 1], w[k + 2]
  std::string parse(const std::vector<std::string>& w, size_t k, const std::string& illegal)
  {
    if (w.size() < k + 3) return illegal;
    if (!chunk_parse_int(w[k], &nevery) || !chunk_parse_int(w[k + 1], &nrepeat) || !chunk_parse_int(w[k + 2], &nfreq)) return illegal;
    if (nevery <= 0 || nrepeat <= 0 || nfreq <= 0) return illegal;
    if (nfreq % nevery || nrepeat * nevery > nfreq) return illegal;
    return std::string();
  }
  // the fix is defined at step t0
  void begin(long long t0) { nvalid = ave_first_valid(t0, nevery, nrepeat, nfreq, start); }
  // A sample step has passed without a sample (steps taken outside run_steps): a new output begins at `step`.  true: the
  // samples of the output that was under way are lost, and the caller zeroes its accumulator
  bool catch_up(long long step)
  {
    if (nvalid >= step) return false;
    begin(step);
    const bool partial = irepeat > 0;
    irepeat = 0;
    return partial;
  }
  bool due(long long step) const { return nvalid == step; }
  // a sample was taken at `step`.  true: it was the last one of its output
  bool sampled(long long step)
  {
    if (++irepeat < nrepeat) {
      nvalid = step + nevery;
      return false;
    }
    irepeat = 0;
    nvalid = step + nfreq - (nrepeat - 1) * nevery;
    return true;
  }
  // the first sample step after `step`, asked once the sample due at `step` (if any) was taken
  long long next(long long step) const { return nvalid > step ? nvalid : ave_first_valid(step + 1, nevery, nrepeat, nfreq, start); }
};

// ---- keywords ----

enum AveKey { AK_NOT_MINE, AK_CONSUMED, AK_ERROR };
enum AveMode { AVE_ONE, AVE_RUNNING, AVE_WINDOW };

struct AveFileSpec {
  std::string file;
  bool overwrite = false;
  bool has_title[3] = {false, false, false};
  std::string title[3];
};

// `file F`, `overwrite`, `title1 S`, `title2 S` or `title3 S` at w[*k]: taken, and *k moved behind it
inline AveKey ave_file_keyword(const std::vector<std::string>& w, size_t* k, AveFileSpec* F)
{
  const std::string& key = w[*k];
  const size_t left = w.size() - *k - 1;
  if (key == "overwrite") {
    F->overwrite = true;
    *k += 1;
    return AK_CONSUMED;
  }
  const bool title = key == "title1" || key == "title2" || key == "title3";
  if (key != "file" && !title) return AK_NOT_MINE;
  if (left < 1) return AK_ERROR;
  if (title) {
    const int t = key[5] - '1';
    F->has_title[t] = true;
    F->title[t] = w[*k + 1];
  } else {
    if (w[*k + 1].empty()) return AK_ERROR;
    F->file = w[*k + 1];
  }
  *k += 2;
  return AK_CONSUMED;
}

// `ave one|running|window M` or `start N` at w[*k], of fix ave/time and fix ave/histo
inline AveKey ave_mode_keyword(const std::vector<std::string>& w, size_t* k, int* ave, long* window, long* start)
{
  const std::string& key = w[*k];
  const size_t left = w.size() - *k - 1;
  if (key == "start") {
    if (left < 1 || !chunk_parse_int(w[*k + 1], start) || *start < 0) return AK_ERROR;
    *k += 2;
    return AK_CONSUMED;
  }
  if (key != "ave") return AK_NOT_MINE;
  if (left < 1) return AK_ERROR;
  if (w[*k + 1] == "one") *ave = AVE_ONE, *k += 2;
  else if (w[*k + 1] == "running") *ave = AVE_RUNNING, *k += 2;
  else if (w[*k + 1] == "window") {
    if (left < 2 || !chunk_parse_int(w[*k + 2], window) || *window <= 0 || *window > 100000) return AK_ERROR;
    *ave = AVE_WINDOW;
    *k += 3;
  } else
    return AK_ERROR;
  return AK_CONSUMED;
}

// ---- the output file ----

// Opened "w+" with its title lines; then one block per output, appended, or under `overwrite` written over the one before
class AveFile {
 public:
  AveFile() = default;
  AveFile(const AveFile&) = delete;
  AveFile& operator=(const AveFile&) = delete;
  ~AveFile()
  {
    if (fp_) fclose(fp_);
  }
  // `style` as in "ave/chunk"; the title lines of S where given, else defaults[0 .. ntitles - 1].  No `file` keyword: nothing
  std::string open(const AveFileSpec& S, const std::string& style, const std::string& id, const std::string* defaults, int ntitles)
  {
    if (S.file.empty()) return std::string();
    fp_ = fopen(S.file.c_str(), "w+");
    if (!fp_) return "Cannot open fix " + style + " file " + S.file;
    who_ = "fix " + style + " " + id;
    path_ = S.file;
    overwrite_ = S.overwrite;
    for (int t = 0; t < ntitles; t++) fprintf(fp_, "%s\n", (S.has_title[t] ? S.title[t] : defaults[t]).c_str());
    fflush(fp_);
    pos_ = ftell(fp_);
    return std::string();
  }
  FILE* fp() const { return fp_; }   // nullptr: no file
  std::string begin_block()
  {
    if (overwrite_ && fseek(fp_, pos_, SEEK_SET) != 0) return who_ + ": cannot rewind " + path_;
    return std::string();
  }
  std::string end_block()
  {
    if (fflush(fp_) != 0) return who_ + ": error writing " + path_;
    if (overwrite_) {
      const long end = ftell(fp_);
      if (end < 0 || ftruncate(fileno(fp_), end) != 0) return who_ + ": cannot truncate " + path_;
    }
    return std::string();
  }

 private:
  FILE* fp_ = nullptr;
  long pos_ = 0;   // behind the titles
  bool overwrite_ = false;
  std::string who_, path_;
};

}  // namespace sf
