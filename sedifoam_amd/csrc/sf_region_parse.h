// sf_region_parse.h -- the words of `region ID style args [side in|out] units box` and `region ID delete`, the table of
// the regions of one engine and the flattening of union / intersect trees into the program of sf_region_match.h (the rules
// of DESIGN.md section 18; [3P] LAMMPS names, rules and error texts: Region, RegBlock, RegSphere, RegCylinder, RegPlane,
// RegUnion, RegIntersect), on the host with nothing but the standard library, so that this code can be compiled into a
// stand-alone program and run under the host sanitizers (sf_displace_parse.h is the precedent; sf_chunk_parse.h holds
// chunk_parse_double).  Every function returns an empty string, or the error text.
#pragma once
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "sf_chunk_parse.h"
#include "sf_region_match.h"

namespace sf {

constexpr int kRegionMax = 32;   // regions of one engine

struct RegionDef {
  std::string id;
  int style = RS_BLOCK;
  std::vector<std::string> subs;   // RS_UNION, RS_INTERSECT: the sub-regions as typed
  RegionProgram prog;              // flat, its own side applied
};

struct RegionTable {
  std::vector<RegionDef> regs;
  const RegionDef* find(const std::string& id) const
  {
    for (const RegionDef& r : regs)
      if (r.id == id) return &r;
    return nullptr;
  }
};

// the box at the moment of the definition (EDGE)
struct RegionBox {
  bool exists = false;
  double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
};

// a bound of a block or of a cylinder's axis: a number, INF or EDGE.  dim 0 1 2, upper: the hi bound
inline std::string region_parse_bound(const std::string& s, const RegionBox& B, int dim, bool upper, const char* illegal, double* v)
{
  if (s == "INF" || s == "EDGE") {
    if (!B.exists) return "Cannot use region INF or EDGE when box does not exist";
    if (s == "INF") *v = upper ? kRegionBig : -kRegionBig;
    else *v = upper ? B.hi[dim] : B.lo[dim];
    return std::string();
  }
  if (!chunk_parse_double(s, v)) return illegal;
  return std::string();
}

// the program of a union (any) or intersect (all) of flat programs, this region's side applied last
inline std::string region_flatten(const std::string& id, const std::vector<const RegionProgram*>& subs, bool all, bool side_out,
                                  RegionProgram* out)
{
  RegionProgram P = RegionProgram();
  for (size_t k = 0; k < subs.size(); k++) {
    const RegionProgram& S = *subs[k];
    if (P.nprim + S.nprim > kRegionMaxPrims)
      return "region " + id + ": more than 16 primitives after flattening its sub-regions";
    if (P.nstep + S.nstep + 2 > kRegionMaxSteps) return "region " + id + ": more than 64 steps after flattening its sub-regions";
    for (int s = 0; s < S.nstep; s++) {
      const int op = S.step[s];
      P.step[P.nstep++] = op < kRegionMaxPrims ? op + P.nprim : op;
    }
    for (int q = 0; q < S.nprim; q++) P.prim[P.nprim + q] = S.prim[q];
    P.nprim += S.nprim;
    if (k > 0) P.step[P.nstep++] = all ? RP_AND : RP_OR;
  }
  if (side_out) P.step[P.nstep++] = RP_NOT;
  *out = P;
  return std::string();
}

// w = region ID delete.  in_use: the regions the dynamic groups test
inline std::string region_delete(RegionTable& T, const std::vector<std::string>& w, const std::vector<std::string>& in_use)
{
  if (w.size() != 3) return "Illegal region command";
  const std::string& id = w[1];
  size_t at = T.regs.size();
  for (size_t k = 0; k < T.regs.size(); k++)
    if (T.regs[k].id == id) at = k;
  if (at == T.regs.size()) return "Delete region ID does not exist";
  for (const std::string& u : in_use)
    if (u == id) return "region " + id + " delete: a dynamic group uses it (group ID static first)";
  for (const RegionDef& r : T.regs)
    for (const std::string& s : r.subs)
      if (s == id) return "region " + id + " delete: region " + r.id + " is a union or intersect of it";
  T.regs.erase(T.regs.begin() + (long)at);
  return std::string();
}

// w = region ID style args [side in|out] units box, or region ID delete
inline std::string region_define(RegionTable& T, const std::vector<std::string>& w, const RegionBox& B,
                                 const std::vector<std::string>& in_use = std::vector<std::string>())
{
  const char* illegal = "Illegal region command";
  if (w.size() < 3 || w[0] != "region") return illegal;
  if (w[2] == "delete") return region_delete(T, w, in_use);
  const std::string& id = w[1];
  const std::string& style = w[2];
  if (T.find(id)) return "Reuse of region ID";
  if (style == "prism" || style == "cone") return "region style " + style + " is not supported (block, sphere, cylinder, plane, union, intersect are)";
  RegionDef R;
  R.id = id;
  RegionPrim p = RegionPrim();
  size_t iarg = 0;   // the first optional keyword
  bool all = false;
  std::vector<const RegionProgram*> subs;
  if (style == "block") {
    illegal = "Illegal region block command";
    if (w.size() < 9) return illegal;
    p.style = R.style = RS_BLOCK;
    for (int k = 0; k < 6; k++) {
      const std::string e = region_parse_bound(w[3 + k], B, k / 2, (k & 1) != 0, illegal, &p.a[k]);
      if (!e.empty()) return e;
    }
    if (p.a[0] > p.a[1] || p.a[2] > p.a[3] || p.a[4] > p.a[5]) return illegal;
    iarg = 9;
  } else if (style == "sphere") {
    illegal = "Illegal region sphere command";
    if (w.size() < 7) return illegal;
    p.style = R.style = RS_SPHERE;
    for (int k = 0; k < 4; k++)
      if (!chunk_parse_double(w[3 + k], &p.a[k])) return illegal;
    if (p.a[3] < 0.0) return illegal;
    iarg = 7;
  } else if (style == "cylinder") {
    illegal = "Illegal region cylinder command";
    if (w.size() < 9) return illegal;
    p.style = R.style = RS_CYLINDER;
    if (w[3] == "x") p.axis = 0;
    else if (w[3] == "y") p.axis = 1;
    else if (w[3] == "z") p.axis = 2;
    else return illegal;
    for (int k = 0; k < 3; k++)
      if (!chunk_parse_double(w[4 + k], &p.a[k])) return illegal;
    if (p.a[2] < 0.0) return illegal;
    for (int k = 0; k < 2; k++) {
      const std::string e = region_parse_bound(w[7 + k], B, p.axis, k == 1, illegal, &p.a[3 + k]);
      if (!e.empty()) return e;
    }
    if (p.a[3] > p.a[4]) return illegal;
    iarg = 9;
  } else if (style == "plane") {
    illegal = "Illegal region plane command";
    if (w.size() < 9) return illegal;
    p.style = R.style = RS_PLANE;
    for (int k = 0; k < 6; k++)
      if (!chunk_parse_double(w[3 + k], &p.a[k])) return illegal;
    // the normal has length one from here on ([3P] RegPlane::RegPlane)
    const double rsq = p.a[3] * p.a[3] + p.a[4] * p.a[4] + p.a[5] * p.a[5];
    if (!(rsq > 0.0) || rsq - rsq != 0.0) return illegal;
    const double len = std::sqrt(rsq);
    for (int k = 3; k < 6; k++) p.a[k] /= len;
    iarg = 9;
  } else if (style == "union" || style == "intersect") {
    all = style == "intersect";
    R.style = all ? RS_INTERSECT : RS_UNION;
    if (w.size() < 4) return illegal;
    char* end = nullptr;
    const long n = std::strtol(w[3].c_str(), &end, 10);
    if (end == w[3].c_str() || *end != '\0' || n < 2 || n > kRegionMaxPrims) return illegal;
    if (w.size() < 4 + (size_t)n) return illegal;
    for (long k = 0; k < n; k++) {
      const RegionDef* s = T.find(w[4 + (size_t)k]);
      if (!s) return all ? "Region intersect region ID does not exist" : "Region union region ID does not exist";
      R.subs.push_back(s->id);
      subs.push_back(&s->prog);
    }
    iarg = 4 + (size_t)n;
  } else
    return "Unknown region style";
  // ---- the optional keywords ([3P] Region::options) ----
  illegal = "Illegal region command";
  bool side_out = false;
  int units = -1;   // 0 box
  while (iarg < w.size()) {
    const std::string& k = w[iarg];
    if (k == "move" || k == "rotate")
      return "region keyword " + k + " is not supported (it needs variables, which this engine does not have)";
    if (k == "open") return "region keyword open is not supported";
    if (iarg + 2 > w.size()) return illegal;
    if (k == "side") {
      if (w[iarg + 1] == "in") side_out = false;
      else if (w[iarg + 1] == "out") side_out = true;
      else return illegal;
    } else if (k == "units") {
      if (w[iarg + 1] == "box") units = 0;
      else if (w[iarg + 1] == "lattice")
        return "region: units lattice is not supported (there is no lattice command): give units box";
      else return illegal;
    } else
      return illegal;
    iarg += 2;
  }
  if (units != 0) return "region: give units box: LAMMPS' default is units lattice, and there is no lattice command";
  if (T.regs.size() >= (size_t)kRegionMax) return "Too many regions (at most 32)";
  if (R.style == RS_UNION || R.style == RS_INTERSECT) {
    const std::string e = region_flatten(id, subs, all, side_out, &R.prog);
    if (!e.empty()) return e;
  } else {
    R.prog = RegionProgram();
    p.side_out = side_out ? 1 : 0;
    R.prog.nprim = 1;
    R.prog.nstep = 1;
    R.prog.step[0] = 0;
    R.prog.prim[0] = p;
  }
  T.regs.push_back(R);
  return std::string();
}

}  // namespace sf
