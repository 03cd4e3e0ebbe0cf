// region_parse_check.cpp -- the host-only parser and region table of csrc/sf_region_parse.h and the predicate of
// csrc/sf_region_match.h over well- and ill-formed lines, the flattening of nested unions and the boundary points of every
// primitive, as a stand-alone program for the host sanitizers (tests/test_region_parse.py builds it with
// -fsanitize=address,undefined -ffp-contract=off and runs it once).  Prints one line per case; exit status 0 when every case
// gave what is expected of it.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_region_parse.h"

namespace {
int failures = 0;

void expect(bool ok, const std::string& what, const std::string& got)
{
  std::printf("%s %s -> %s\n", ok ? "ok  " : "FAIL", what.c_str(), got.empty() ? "(accepted)" : got.c_str());
  if (!ok) failures++;
}

std::string define(sf::RegionTable& T, const std::string& line, const sf::RegionBox& B,
                   const std::vector<std::string>& in_use = std::vector<std::string>())
{
  std::vector<std::string> w;
  std::string e = sf::split_quoted(line, &w);
  if (e.empty()) e = sf::region_define(T, w, B, in_use);
  return e;
}

void good(sf::RegionTable& T, const std::string& line, const sf::RegionBox& B)
{
  const size_t n = T.regs.size();
  const std::string e = define(T, line, B);
  expect(e.empty() && T.regs.size() == n + 1, line, e);
}

void bad(sf::RegionTable& T, const std::string& line, const sf::RegionBox& B, const std::string& text,
         const std::vector<std::string>& in_use = std::vector<std::string>())
{
  const size_t n = T.regs.size();
  const std::string e = define(T, line, B, in_use);
  expect(e.find(text) != std::string::npos && T.regs.size() == n, line, e);
}

bool match(const sf::RegionTable& T, const char* id, double x, double y, double z)
{
  const sf::RegionDef* d = T.find(id);
  if (!d) {
    failures++;
    std::printf("FAIL no region %s\n", id);
    return false;
  }
  return sf::region_match(d->prog, x, y, z);
}

void point(const sf::RegionTable& T, const char* id, double x, double y, double z, bool want)
{
  char what[160];
  std::snprintf(what, sizeof what, "match %s (%.17g %.17g %.17g) = %d", id, x, y, z, (int)want);
  expect(match(T, id, x, y, z) == want, what, "");
}
}  // namespace

int main()
{
  sf::RegionBox none, B;
  B.exists = true;
  B.lo[0] = 0.0; B.hi[0] = 4.0;
  B.lo[1] = -1.0; B.hi[1] = 2.0;
  B.lo[2] = 0.5; B.hi[2] = 8.0;
  sf::RegionTable T;
  // ---- well-formed lines of every style and keyword ----
  good(T, "region b block 0 1 0 2 0.25 3 units box", B);
  good(T, "region bo block 0 1 0 2 0.25 3 side out units box", B);
  good(T, "region bi block 0 1 0 2 0.25 3 units box side in", B);
  good(T, "region be block EDGE EDGE INF INF EDGE INF units box", B);
  good(T, "region s sphere 1 1 1 3 units box", B);
  good(T, "region s7 sphere 0 0 0 7 side out units box", B);
  good(T, "region cx cylinder x 1 2 5 0 1 units box", B);
  good(T, "region cy cylinder y 1 2 5 0 1 units box", B);
  good(T, "region cz cylinder z 1 2 5 INF EDGE units box", B);
  good(T, "region p plane 1 0 0 2 0 0 units box", B);
  good(T, "region pd plane 0 1 0 0 -4 0 units box   # a comment", B);
  good(T, "region u union 2 b s units box", B);
  good(T, "region i intersect 2 b s7 units box", B);
  good(T, "region n union 2 i bo side out units box", B);
  good(T, "region pre block 0 1 0 1 0 1 units box", none);   // (numbers need no box)
  {
    const sf::RegionDef* d = T.find("be");
    const double want[6] = {0.0, 4.0, -sf::kRegionBig, sf::kRegionBig, 0.5, sf::kRegionBig};
    bool same = d != nullptr;
    for (int k = 0; same && k < 6; k++) same = d->prog.prim[0].a[k] == want[k];
    expect(same, "EDGE is the box bound, INF is -+1e20", "");
    d = T.find("cz");
    expect(d && d->prog.prim[0].axis == 2 && d->prog.prim[0].a[3] == -sf::kRegionBig && d->prog.prim[0].a[4] == 8.0,
           "cylinder z lo INF hi EDGE", "");
    d = T.find("p");
    expect(d && d->prog.prim[0].a[3] == 1.0 && d->prog.prim[0].a[4] == 0.0 && d->prog.prim[0].a[5] == 0.0,
           "the plane's normal is normalised at the definition", "");
  }
  // ---- ill-formed lines, each with its text ----
  bad(T, "region", B, "Illegal region command");
  bad(T, "region x", B, "Illegal region command");
  bad(T, "region b block 0 1 0 1 0 1 units box", B, "Reuse of region ID");
  bad(T, "region x block 0 1 0 1 0 1", B, "give units box");
  bad(T, "region x block 0 1 0 1 0 1 units lattice", B, "units lattice is not supported");
  bad(T, "region x block 0 1 0 1 0 1 units", B, "Illegal region command");
  bad(T, "region x block 0 1 0 1 0 1 units reduced", B, "Illegal region command");
  bad(T, "region x block 0 1 0 1 0 1 side up units box", B, "Illegal region command");
  bad(T, "region x block 0 1 0 1 0 1 colour red units box", B, "Illegal region command");
  bad(T, "region x block 1 0 0 1 0 1 units box", B, "Illegal region block command");
  bad(T, "region x block 0 1 0 1 0 units box", B, "Illegal region block command");
  bad(T, "region x block 0 1 0 1 0", B, "Illegal region block command");
  bad(T, "region x block 0 1 0 1 0 1x units box", B, "Illegal region block command");
  bad(T, "region x block 0 1 0 nan 0 1 units box", B, "Illegal region block command");
  bad(T, "region x block 0 inf 0 1 0 1 units box", B, "Illegal region block command");
  bad(T, "region x block INF 1 0 1 0 1 units box", none, "Cannot use region INF or EDGE when box does not exist");
  bad(T, "region x block 0 EDGE 0 1 0 1 units box", none, "Cannot use region INF or EDGE when box does not exist");
  bad(T, "region x cylinder z 0 0 1 EDGE 1 units box", none, "Cannot use region INF or EDGE when box does not exist");
  bad(T, "region x sphere 0 0 0 units box", B, "Illegal region sphere command");
  bad(T, "region x sphere 0 0 0 -1 units box", B, "Illegal region sphere command");
  bad(T, "region x sphere 0 0 INF 1 units box", B, "Illegal region sphere command");
  bad(T, "region x cylinder w 0 0 1 0 1 units box", B, "Illegal region cylinder command");
  bad(T, "region x cylinder z 0 0 1 1 0 units box", B, "Illegal region cylinder command");
  bad(T, "region x cylinder z 0 0 -1 0 1 units box", B, "Illegal region cylinder command");
  bad(T, "region x cylinder z 0 0 1 0", B, "Illegal region cylinder command");
  bad(T, "region x plane 0 0 0 0 0 0 units box", B, "Illegal region plane command");
  bad(T, "region x plane 0 0 0 1 0 units box", B, "Illegal region plane command");
  bad(T, "region x plane 0 0 0 1 0 1e units box", B, "Illegal region plane command");
  bad(T, "region x prism 0 1 0 1 0 1 0 0 0 units box", B, "region style prism is not supported");
  bad(T, "region x cone z 0 0 1 2 0 1 units box", B, "region style cone is not supported");
  bad(T, "region x block 0 1 0 1 0 1 move v_a NULL NULL units box", B, "keyword move is not supported");
  bad(T, "region x block 0 1 0 1 0 1 units box rotate v_t 0 0 0 0 0 1", B, "keyword rotate is not supported");
  bad(T, "region x block 0 1 0 1 0 1 open 1 units box", B, "keyword open is not supported");
  bad(T, "region x wedge 0 1 units box", B, "Unknown region style");
  bad(T, "region x union 1 b units box", B, "Illegal region command");
  bad(T, "region x union two b s units box", B, "Illegal region command");
  bad(T, "region x union 3 b s units box", B, "Region union region ID does not exist");   // (`units` is read as the third ID)
  bad(T, "region x union 3 b s", B, "Illegal region command");
  bad(T, "region x union 2 b nosuch units box", B, "Region union region ID does not exist");
  bad(T, "region x intersect 2 nosuch b units box", B, "Region intersect region ID does not exist");
  bad(T, "region x block 0 1 0 1 0 1 units 'box", B, "Unbalanced quotes in input line");
  // ---- delete ----
  bad(T, "region nosuch delete", B, "Delete region ID does not exist");
  bad(T, "region b delete now", B, "Illegal region command");
  bad(T, "region b delete", B, "is a union or intersect of it");             // (u and i use it)
  bad(T, "region i delete", B, "is a union or intersect of it");             // (n uses it)
  bad(T, "region pd delete", B, "a dynamic group uses it", {"p", "pd"});
  {
    const size_t n = T.regs.size();
    std::string e = define(T, "region pd delete", B, {"p"});
    expect(e.empty() && T.regs.size() == n - 1 && !T.find("pd"), "region pd delete", e);
    e = define(T, "region n delete", B);
    expect(e.empty() && !T.find("n"), "region n delete", e);
    e = define(T, "region i delete", B);
    expect(e.empty() && !T.find("i"), "region i delete (no longer used)", e);
    good(T, "region i intersect 2 b s7 units box", B);
    good(T, "region n union 2 i bo side out units box", B);
  }
  // ---- flattening ----
  {
    const sf::RegionDef* d = T.find("n");
    // n = not (((b and s7') or bo')): primitives b s7 bo, steps 0 1 and 2 or not
    const int want[6] = {0, 1, sf::RP_AND, 2, sf::RP_OR, sf::RP_NOT};
    bool same = d && d->prog.nprim == 3 && d->prog.nstep == 6;
    for (int k = 0; same && k < 6; k++) same = d->prog.step[k] == want[k];
    same = same && d->prog.prim[0].style == sf::RS_BLOCK && d->prog.prim[1].style == sf::RS_SPHERE &&
           d->prog.prim[1].side_out == 1 && d->prog.prim[2].side_out == 1;
    expect(same, "the program of a nested union", "");
    // 16 primitives fit, 17 do not: u2 = 2, u4 = 4, u8 = 8, u16 = 16, u17 = u16 + b
    good(T, "region u2 union 2 b s units box", B);
    good(T, "region u4 intersect 2 u2 u2 side out units box", B);
    good(T, "region u8 union 2 u4 u4 units box", B);
    good(T, "region u16 intersect 2 u8 u8 side out units box", B);
    d = T.find("u16");
    expect(d && d->prog.nprim == 16 && d->prog.nstep == 16 + 15 + 5, "16 primitives after flattening", "");
    bad(T, "region u17 union 2 u16 b units box", B, "more than 16 primitives");
    bad(T, "region u17 union 2 b u16 units box", B, "more than 16 primitives");
    bad(T, "region u24 union 3 u8 u8 u8 units box", B, "more than 16 primitives");
    bad(T, "region u17 union 17 b b b b b b b b b b b b b b b b b units box", B, "Illegal region command");
    good(T, "region w16 union 16 b b b b b b b b b b b b b b b s units box", B);
    // the table holds 32 regions
    while (T.regs.size() < (size_t)sf::kRegionMax) good(T, "region f" + std::to_string(T.regs.size()) + " sphere 0 0 0 1 units box", B);
    bad(T, "region toomany sphere 0 0 0 1 units box", B, "Too many regions");
  }
  // ---- region_match on the host, at the boundary points ----
  // block b = [0, 1] x [0, 2] x [0.25, 3], closed: faces, edges, corners are inside; one ulp beyond is not
  point(T, "b", 0.5, 1.0, 0.25, true);
  point(T, "b", 0.0, 1.0, 1.0, true);
  point(T, "b", 1.0, 2.0, 1.0, true);
  point(T, "b", 0.0, 0.0, 0.25, true);
  point(T, "b", 1.0, 2.0, 3.0, true);
  point(T, "b", 1.0000000000000002, 2.0, 3.0, false);
  point(T, "b", 1.0, 2.0, 0.24999999999999997, false);
  point(T, "b", -4.9406564584124654e-324, 1.0, 1.0, false);
  point(T, "bo", 1.0, 2.0, 3.0, false);
  point(T, "bo", 1.0, 2.0, 3.0000000000000004, true);
  point(T, "bi", 1.0, 2.0, 3.0, true);
  point(T, "be", 4.0, -9.0e19, 0.5, true);
  point(T, "be", 4.0, 1.0e21, 0.5, false);
  point(T, "be", 2.0, 0.0, 0.49999999999999994, false);
  // sphere s: centre 1 1 1, r 3; offsets (1 2 2) and permutations: 1 + 4 + 4 = 9
  point(T, "s", 2.0, 3.0, 3.0, true);
  point(T, "s", 3.0, 2.0, -1.0, true);
  point(T, "s", 2.0 + 0x1p-49, 3.0, 3.0, false);
  point(T, "s", 2.0 - 0x1p-49, 3.0, 3.0, true);
  point(T, "s", 4.0, 1.0, 1.0 + 0x1p-20, false);
  // s7: centre 0, r 7, side out; (2 3 6): 4 + 9 + 36 = 49
  point(T, "s7", 2.0, 3.0, 6.0, false);
  point(T, "s7", -6.0, 2.0, -3.0, false);
  point(T, "s7", 2.0, 3.0, 6.5, true);
  // cylinders: c1 c2 = 1 2, r 5, axis range [0, 1]; offsets (3 4): 9 + 16 = 25
  point(T, "cy", 4.0, 0.0, 6.0, true);
  point(T, "cy", 4.0, 1.0, 6.0, true);
  point(T, "cy", 4.0, 1.0000000000000002, 6.0, false);
  point(T, "cy", 4.0, 0.5, 6.0000000000000009, false);
  point(T, "cx", 0.5, 4.0, 6.0, true);
  point(T, "cx", 4.0, 0.5, 6.0, false);
  point(T, "cz", 4.0, 6.0, 8.0, true);
  point(T, "cz", -2.0, -2.0, -1.0e19, true);
  point(T, "cz", 4.0, 6.0, 8.0000000000000018, false);
  // planes: p is x >= 1
  point(T, "p", 1.0, 5.0, 5.0, true);
  point(T, "p", 0.99999999999999989, 5.0, 5.0, false);
  point(T, "p", 1.0e30, -1.0e30, 0.0, true);
  // the nested region n = not ((b and not-in-s7) or not-in-b): inside b only the ball of s7 matters
  point(T, "n", 0.5, 1.0, 1.0, true);      // in b, inside s7's ball: i fails, bo fails -> not -> match
  point(T, "n", 5.0, 5.0, 5.0, false);     // outside b: bo matches -> no match
  point(T, "i", 0.5, 1.0, 1.0, false);
  point(T, "u", 3.9, 1.0, 1.0, true);      // in s, not in b
  point(T, "u16", 0.5, 1.0, 1.0, match(T, "u16", 0.5, 1.0, 1.0));   // (walks the longest program: the sanitizers watch it)
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
