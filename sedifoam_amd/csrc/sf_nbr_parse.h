// sf_nbr_parse.h -- the words of `compute ID group rdf Nbin [itype jtype ...] cutoff Rc`, `compute ID group coord/atom
// cutoff Rc [typerange ...]` and `compute ID group cluster/atom CUT [surface no|yes] [size no|yes]` ([3P] LAMMPS names:
// ComputeRDF::ComputeRDF, ComputeCoordAtom::ComputeCoordAtom, ComputeClusterAtom::ComputeClusterAtom, utils::bounds
// for a type range), on the host with nothing but the standard library, so that this code can be compiled into a stand-alone
// program and run under the host sanitizers (tests/c_abi/nbr_parse_check.cpp; sf_chunk_parse.h is the precedent).  Every
// parser returns an empty string, or the error text.
#pragma once
#include <climits>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "sf_ave_common.h"

namespace sf {

constexpr long kRdfMaxCounters = 8192;   // Nbin * npairs: the bound of fix ave/histo's bins
constexpr int kCoordMaxRanges = 8;       // columns of one compute coord/atom

// types lo .. hi, both ends included.  The engine keeps no type count: an open end is every type from or up to there
struct TypeRange {
  int lo = INT_MIN, hi = INT_MAX;
  bool has(int t) const { return t >= lo && t <= hi; }
};

// digits and nothing else: a type number
inline bool nbr_parse_type(const std::string& s, int* v)
{
  long t = 0;
  if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos || !chunk_parse_int(s, &t)) return false;
  *v = (int)t;
  return true;
}

// an integer, a*b, a*, *b or *
inline bool parse_type_range(const std::string& s, TypeRange* r)
{
  *r = TypeRange();
  const size_t star = s.find('*');
  if (star == std::string::npos) {
    if (!nbr_parse_type(s, &r->lo)) return false;
    r->hi = r->lo;
    return true;
  }
  if (s.find('*', star + 1) != std::string::npos) return false;
  const std::string a = s.substr(0, star), b = s.substr(star + 1);
  if (!a.empty() && !nbr_parse_type(a, &r->lo)) return false;
  if (!b.empty() && !nbr_parse_type(b, &r->hi)) return false;
  return r->lo <= r->hi;
}

// a cutoff: one finite number above zero and nothing behind it
inline bool nbr_parse_cutoff(const std::string& s, double* v)
{
  if (s.empty()) return false;
  char* end = nullptr;
  *v = std::strtod(s.c_str(), &end);
  return end != s.c_str() && *end == '\0' && std::isfinite(*v) && *v > 0.0;
}

struct RdfPair {
  TypeRange i, j;
};

struct RdfSpec {
  std::string id, group;
  long nbin = 1;
  std::vector<RdfPair> pairs;
  double rc = 0.0;
};

// w = compute ID group rdf Nbin [itype jtype ...] cutoff Rc
inline std::string parse_rdf(const std::vector<std::string>& w, RdfSpec* out)
{
  const std::string illegal = "Illegal compute rdf command";
  if (w.size() < 5) return illegal;
  RdfSpec S;
  S.id = w[1];
  S.group = w[2];
  if (!chunk_parse_int(w[4], &S.nbin) || S.nbin < 1) return illegal;
  size_t k = 5;
  while (k < w.size() && w[k] != "cutoff") {
    RdfPair p;
    if (k + 1 >= w.size() || w[k + 1] == "cutoff") return illegal;   // (a type without its partner)
    if (!parse_type_range(w[k], &p.i) || !parse_type_range(w[k + 1], &p.j)) return illegal;
    S.pairs.push_back(p);
    k += 2;
  }
  if (k >= w.size())
    return "compute rdf: the cutoff keyword is required (this engine's pair list ends at the contact distance plus the skin)";
  if (k + 2 != w.size() || !nbr_parse_cutoff(w[k + 1], &S.rc)) return illegal;
  if (S.pairs.empty()) S.pairs.push_back(RdfPair());
  if (S.nbin > kRdfMaxCounters || S.nbin * (long)S.pairs.size() > kRdfMaxCounters)
    return "compute rdf: Nbin * npairs is above 8192 (the bound of fix ave/histo's bins)";
  *out = S;
  return std::string();
}

struct CoordSpec {
  double rc = 0.0;
  std::vector<TypeRange> ranges;
};

// w = compute ID group coord/atom cutoff Rc [typerange ...]
inline std::string parse_coord_atom(const std::vector<std::string>& w, CoordSpec* out)
{
  const std::string illegal = "Illegal compute coord/atom command";
  if (w.size() < 5) return illegal;
  if (w[4] != "cutoff") return "compute coord/atom: only cstyle cutoff is supported (compute ID group coord/atom cutoff Rc [typerange ...])";
  CoordSpec S;
  if (w.size() < 6 || !nbr_parse_cutoff(w[5], &S.rc)) return illegal;
  for (size_t k = 6; k < w.size(); k++) {
    TypeRange r;
    if (!parse_type_range(w[k], &r)) return illegal;
    if ((int)S.ranges.size() >= kCoordMaxRanges) return "compute coord/atom: more than 8 type ranges";
    S.ranges.push_back(r);
  }
  if (S.ranges.empty()) S.ranges.push_back(TypeRange());
  *out = S;
  return std::string();
}

// ---- compute cluster/atom ([3P] LAMMPS name and rule: ComputeClusterAtom) ----

struct ClusterSpec {
  double cut = 0.0;
  bool surface = false;   // [own] linked when rsq < ((ri + rj) + cut)^2: the reach test of fix cohesive
  bool size = false;      // [own] a second column: the atoms of the atom's cluster
};

// w = compute ID group cluster/atom CUT [surface no|yes] [size no|yes]
inline std::string parse_cluster_atom(const std::vector<std::string>& w, ClusterSpec* out)
{
  const std::string illegal = "Illegal compute cluster/atom command";
  if (w.size() < 5) return illegal;
  ClusterSpec S;
  char* end = nullptr;
  S.cut = w[4].empty() ? 0.0 : std::strtod(w[4].c_str(), &end);
  if (w[4].empty() || end == w[4].c_str() || *end != '\0' || !std::isfinite(S.cut)) return illegal;
  for (size_t k = 5; k < w.size(); k += 2) {
    if (k + 1 >= w.size() || (w[k + 1] != "no" && w[k + 1] != "yes")) return illegal;
    const bool yes = w[k + 1] == "yes";
    if (w[k] == "surface") S.surface = yes;
    else if (w[k] == "size") S.size = yes;
    else return illegal;
  }
  // (a centre distance below zero links nothing and makes no grid; a gap of zero between surfaces is touching)
  if (S.surface ? !(S.cut >= 0.0) : !(S.cut > 0.0)) return illegal;
  *out = S;
  return std::string();
}

// the bond-based siblings of cluster/atom, refused by name; empty: `style` is neither
inline std::string cluster_unsupported_style(const std::string& style)
{
  if (style == "fragment/atom" || style == "aggregate/atom")
    return "compute " + style + " is not supported (there are no bonds; cluster/atom is)";
  return std::string();
}

}  // namespace sf
