// sf_global_parse.h -- the words of `compute ID group reduce MODE input ...`, `compute ID group property/atom attr ...`,
// `fix ID group ave/time Nevery Nrepeat Nfreq value ... keywords` and a `c_ID` / `c_ID[k]` column of thermo_style custom
// ([3P] LAMMPS names and rules: ComputeReduce::ComputeReduce, ComputePropertyAtom, FixAveTime::FixAveTime / options /
// nextvalid, Thermo::parse_fields), on the host with nothing but the standard library, so that this code can be compiled
// into a stand-alone program and run under the host sanitizers (sf_chunk_parse.h is the precedent, and holds split_quoted
// and ave_format_ok; the schedule, the file, ave and start keywords, the attribute words and parse_cref are those of
// sf_ave_common.h).  Every parser returns an empty string, or the error text.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sf_chunk_parse.h"

namespace sf {

// ---- compute reduce ----

enum GlobalMode { GM_SUM, GM_MIN, GM_MAX, GM_AVE, GM_SUMSQ, GM_AVESQ };
constexpr int kReduceMaxInputs = 64;

struct ReduceInput {
  int attr = AA_X;
  std::string word;   // as typed
  std::string id;     // AA_COMPUTE
  long index = 0;     // AA_COMPUTE: k of c_ID[k], 0: none
};

struct ReduceSpec {
  std::string id, group;
  int mode = GM_SUM;
  std::vector<ReduceInput> inputs;
};

// w = compute ID group reduce MODE input ...
inline std::string parse_reduce(const std::vector<std::string>& w, ReduceSpec* out)
{
  const std::string illegal = "Illegal compute reduce command";
  if (w.size() < 6) return illegal;
  ReduceSpec S;
  S.id = w[1];
  S.group = w[2];
  static const char* const modes[6] = {"sum", "min", "max", "ave", "sumsq", "avesq"};
  int mode = -1;
  for (int q = 0; q < 6; q++)
    if (w[4] == modes[q]) mode = q;
  if (w[4] == "sumabs" || w[4] == "aveabs" || w[4] == "minabs" || w[4] == "maxabs")
    return "compute reduce: mode " + w[4] + " is not supported (sum, min, max, ave, sumsq and avesq are)";
  if (mode < 0) return illegal;
  S.mode = mode;
  for (size_t k = 5; k < w.size(); k++) {
    const std::string& s = w[k];
    ReduceInput in;
    in.word = s;
    const int a = ave_attr_of(s);
    if (a >= 0) in.attr = a;
    else if (s == "replace" || s == "inputs")
      return "compute reduce: keyword " + s + " is not supported";
    else if (s.compare(0, 2, "f_") == 0 || s.compare(0, 2, "v_") == 0)
      return "compute reduce: " + s + " is not supported (f_ and v_ inputs are not; x y z vx vy vz fx fy fz, c_ID and c_ID[k] are)";
    else if (s.compare(0, 2, "c_") == 0) {
      in.attr = AA_COMPUTE;
      if (!parse_cref(s, &in.id, &in.index)) return illegal;
    } else
      return illegal;
    if ((int)S.inputs.size() >= kReduceMaxInputs) return "compute reduce: more than 64 inputs";
    S.inputs.push_back(in);
  }
  *out = S;
  return std::string();
}

// ---- compute cluster/stats [own] ----

// w = compute ID group cluster/stats CID, CID the ID of a compute cluster/atom
inline std::string parse_cluster_stats(const std::vector<std::string>& w, std::string* cid)
{
  if (w.size() != 5 || w[4].empty()) return "Illegal compute cluster/stats command";
  if (w[4].compare(0, 2, "c_") == 0)
    return "compute cluster/stats: give the ID of the cluster/atom compute itself (" + w[4].substr(2) + ", not " + w[4] + ")";
  *cid = w[4];
  return std::string();
}

// ---- compute property/atom ----

enum PropAttr {
  PA_ID, PA_TYPE, PA_MASS, PA_RADIUS, PA_DIAMETER, PA_X, PA_Y, PA_Z, PA_VX, PA_VY, PA_VZ, PA_FX, PA_FY, PA_FZ, PA_OMEGAX,
  PA_OMEGAY, PA_OMEGAZ, PA_TQX, PA_TQY, PA_TQZ,
  PA_COUNT,   // the attributes a state record holds as stored
  // derived from the record and the periodic image counts (sf_unmap.h): unwrapped coordinates, and the counts themselves
  PA_XU = PA_COUNT, PA_YU, PA_ZU, PA_IX, PA_IY, PA_IZ,
  PA_COUNT_ALL
};
constexpr int kPropMaxAttrs = 24;

inline const char* prop_attr_name(int a)
{
  static const char* const names[PA_COUNT_ALL] = {"id", "type", "mass", "radius", "diameter", "x", "y", "z", "vx", "vy",
                                                  "vz", "fx", "fy", "fz", "omegax", "omegay", "omegaz", "tqx", "tqy", "tqz",
                                                  "xu", "yu", "zu", "ix", "iy", "iz"};
  return a >= 0 && a < PA_COUNT_ALL ? names[a] : "";
}
inline bool prop_attr_needs_image(int a) { return a >= PA_XU && a <= PA_IZ; }

// w = compute ID group property/atom a1 ...
inline std::string parse_property_atom(const std::vector<std::string>& w, std::vector<int>* attrs)
{
  if (w.size() < 5) return "Illegal compute property/atom command";
  attrs->clear();
  for (size_t k = 4; k < w.size(); k++) {
    int a = -1;
    for (int q = 0; q < PA_COUNT_ALL; q++)
      if (w[k] == prop_attr_name(q)) a = q;
    if (a < 0) return "Invalid keyword in compute property/atom command: " + w[k];
    if ((int)attrs->size() >= kPropMaxAttrs) return "compute property/atom: more than 24 attributes";
    attrs->push_back(a);
  }
  return std::string();
}

// ---- fix ave/time ----

constexpr int kAveTimeMaxValues = 64;

struct AveTimeValue {
  std::string word, id;
  long index = 0;
};

struct AveTimeSpec : AveSchedule, AveFileSpec {   // (title3 belongs to mode vector: accepted and unused in mode scalar)
  std::string id, group;
  std::vector<AveTimeValue> values;
  bool mode_vector = false;   // the values are columns c_ID[k] of global arrays with one row count (compute rdf)
  int ave = AVE_ONE;
  long window = 0;
  std::string format = " %g";
};

// a format of fix ave/time: blanks, then one conversion of a double (ave_format_ok)
inline bool ave_time_format_ok(const std::string& f)
{
  size_t k = 0;
  while (k < f.size() && f[k] == ' ') k++;
  return k <= 8 && ave_format_ok(f.substr(k));
}

// w = fix ID group ave/time Nevery Nrepeat Nfreq value ... keywords (split_quoted words)
inline std::string parse_ave_time(const std::vector<std::string>& w, AveTimeSpec* out)
{
  const std::string illegal = "Illegal fix ave/time command";
  if (w.size() < 8) return illegal;
  AveTimeSpec S;
  S.id = w[1];
  S.group = w[2];
  if (!S.parse(w, 4, illegal).empty()) return illegal;
  size_t k = 7;
  for (; k < w.size(); k++) {
    const std::string& s = w[k];
    if (s.compare(0, 2, "f_") == 0 || s.compare(0, 2, "v_") == 0)
      return "fix ave/time: " + s + " is not supported (f_ and v_ values are not; c_ID and c_ID[k] of a global compute are)";
    if (s.compare(0, 2, "c_") != 0) break;
    AveTimeValue v;
    v.word = s;
    if (!parse_cref(s, &v.id, &v.index)) return illegal;
    if ((int)S.values.size() >= kAveTimeMaxValues) return "fix ave/time: more than 64 values";
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
      if (w[k + 1] != "scalar" && w[k + 1] != "vector") return illegal;
      S.mode_vector = w[k + 1] == "vector";
      k += 2;
    } else if (key == "off") {
      return "fix ave/time: off is not supported (mode vector takes whole columns of a global array)";
    } else if (key == "format") {
      if (left < 1) return illegal;
      if (!ave_time_format_ok(w[k + 1]))
        return "fix ave/time: format " + w[k + 1] + " is not one %g-class conversion of a double (such as \" %.10g\")";
      S.format = w[k + 1];
      k += 2;
    } else
      return illegal;
  }
  if (S.mode_vector)
    for (const AveTimeValue& v : S.values)
      if (v.index == 0)
        return "fix ave/time: mode vector is not supported for " + v.word + " (a global vector is not taken; c_ID[k], a column "
               "of a global array such as compute rdf, is)";
  *out = S;
  return std::string();
}

// ---- mode vector: the text of one output ----

// title3 of mode vector where none is given
inline std::string ave_time_title3(const AveTimeSpec& S)
{
  std::string t = "# Row";
  for (const AveTimeValue& v : S.values) t += " " + v.word;
  return t;
}

// ---- thermo_style custom ... c_ID c_ID[k] ----

inline std::string parse_thermo_column(const std::string& word, std::string* id, long* index)
{
  if (!parse_cref(word, id, index)) return "Invalid keyword in thermo_style custom command: " + word;
  return std::string();
}

}  // namespace sf
