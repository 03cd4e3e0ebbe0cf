// sf_displace_parse.h -- the words of `compute ID group displace/atom` and `compute ID group com` ([3P] LAMMPS names and
// rules: ComputeDisplaceAtom, ComputeCOM), on the host with
// nothing but the standard library, so that this code can be compiled into a stand-alone program and run under the host
// sanitizers (sf_global_parse.h is the precedent; it holds the attribute names xu yu zu ix iy iz of compute
// property/atom).  Every parser returns an empty string, or the error text.
#pragma once
#include <string>
#include <vector>

namespace sf {

// w = compute ID group displace/atom
inline std::string parse_displace_atom(const std::vector<std::string>& w)
{
  if (w.size() != 4) return "Illegal compute displace/atom command";
  return std::string();
}

// w = compute ID group com
inline std::string parse_com(const std::vector<std::string>& w)
{
  if (w.size() != 4) return "Illegal compute com command";
  return std::string();
}

}  // namespace sf
