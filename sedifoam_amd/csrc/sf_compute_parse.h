// sf_compute_parse.h -- the words of the per-atom computes, parsed on the host with nothing but the standard library (so
// that this code can be compiled into a stand-alone program and run under the host sanitizers):
//   a dump column `c_ID` / `c_ID[k]`                                  ([3P] DumpCustom::parse_fields)
//   the keywords of `compute ID group stress/atom [NULL] [ke] ...`    ([3P] ComputeStressAtom::ComputeStressAtom)
// Both return an empty string, or the error text.
#pragma once
#include <string>
#include <vector>

#include "sf_ave_common.h"

namespace sf {

// `word` = c_ID or c_ID[k]: the ID and k (0: no index given), by parse_cref of sf_ave_common.h
inline std::string parse_compute_column(const std::string& word, const char* dump_style, std::string* id, long* index)
{
  const std::string bad = "Invalid attribute " + word + " in dump " + dump_style + " command";
  return parse_cref(word, id, index) ? std::string() : bad;
}

// w[first ...]: the words behind `stress/atom`.  No keyword: ke and pair both; `virial` = `pair`; fix bond angle dihedral
// improper kspace are accepted and add nothing here; a leading NULL (the temp-ID of later LAMMPS versions) is skipped
inline std::string parse_stress_keywords(const std::vector<std::string>& w, size_t first, bool* ke, bool* pair)
{
  auto zero = [](const std::string& s) {
    return s == "fix" || s == "bond" || s == "angle" || s == "dihedral" || s == "improper" || s == "kspace";
  };
  size_t k = first;
  if (k < w.size() && w[k] == "NULL") k++;
  if (k >= w.size()) {
    *ke = *pair = true;
    return std::string();
  }
  *ke = *pair = false;
  for (; k < w.size(); k++) {
    if (w[k] == "ke") *ke = true;
    else if (w[k] == "pair" || w[k] == "virial") *pair = true;
    else if (zero(w[k])) {
      // no fix here tallies a virial and there are no bonded or long-range terms: zero
    } else if (k == first)   // where later LAMMPS versions take a temperature compute
      return "compute stress/atom: a temperature compute (" + w[k] + ") is not supported by this engine (NULL is)";
    else
      return "Illegal compute stress/atom command";
  }
  return std::string();
}

}  // namespace sf
