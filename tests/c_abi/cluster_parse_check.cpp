// cluster_parse_check.cpp -- parse_cluster_atom of csrc/sf_nbr_parse.h and the words of compute cluster/stats of
// csrc/sf_global_parse.h (both host-only) over well- and ill-formed lines, as a stand-alone program for the host sanitizers
// (tests/test_cluster_parse.py builds it with -fsanitize=address,undefined and runs it once).  Prints one line per case;
// exit status 0 when every case gave what is expected of it.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_global_parse.h"
#include "../../sedifoam_amd/csrc/sf_nbr_parse.h"

namespace {
int failures = 0;

void expect(bool ok, const std::string& what, const std::string& got)
{
  std::printf("%s %s -> %s\n", ok ? "ok  " : "FAIL", what.c_str(), got.empty() ? "(accepted)" : got.c_str());
  if (!ok) failures++;
}

std::vector<std::string> words(const std::string& line)
{
  std::vector<std::string> w;
  sf::split_quoted(line, &w);
  return w;
}

void cluster_ok(const std::string& args, double cut, bool surface, bool size)
{
  sf::ClusterSpec S;
  const std::string e = sf::parse_cluster_atom(words("compute cl all cluster/atom " + args), &S);
  expect(e.empty() && S.cut == cut && S.surface == surface && S.size == size, "cluster/atom " + args, e);
}

void cluster_bad(const std::string& args)
{
  sf::ClusterSpec S;
  S.cut = -7.0;
  const std::string e = sf::parse_cluster_atom(words("compute cl all cluster/atom " + args), &S);
  // (what is refused leaves the caller's spec alone)
  expect(e == "Illegal compute cluster/atom command" && S.cut == -7.0 && !S.surface && !S.size, "cluster/atom " + args, e);
}

void stats_ok(const std::string& args, const std::string& cid)
{
  std::string got;
  const std::string e = sf::parse_cluster_stats(words("compute st all cluster/stats " + args), &got);
  expect(e.empty() && got == cid, "cluster/stats " + args, e);
}

void stats_bad(const std::string& line, const std::string& part)
{
  std::string got = "untouched";
  const std::string e = sf::parse_cluster_stats(words(line), &got);
  expect(!e.empty() && e.find(part) != std::string::npos && got == "untouched", line, e);
}
}  // namespace

int main()
{
  // ---- compute cluster/atom ----
  cluster_ok("1.1e-3", 1.1e-3, false, false);   // (the bare LAMMPS form)
  cluster_ok("2", 2.0, false, false);
  cluster_ok("0x1p-8", 0x1p-8, false, false);
  cluster_ok("1e-3 surface no", 1e-3, false, false);
  cluster_ok("1e-3 surface yes", 1e-3, true, false);
  cluster_ok("0 surface yes", 0.0, true, false);   // (a gap of zero: touching)
  cluster_ok("0.0 size yes surface yes", 0.0, true, true);
  cluster_ok("1e-3 size yes", 1e-3, false, true);
  cluster_ok("1e-3 size no", 1e-3, false, false);
  cluster_ok("1e-3 surface yes size yes", 1e-3, true, true);
  cluster_ok("1e-3 size yes surface no", 1e-3, false, true);
  cluster_ok("1e-3 surface yes surface no", 1e-3, false, false);   // (the last one holds, as in LAMMPS' keyword loops)
  for (const char* s : {"", "cutoff 1e-3", "0", "0.0", "-0.0", "-1e-3", "-1e-3 surface yes", "0 surface no", "0 size yes", "nan",
                        "nan surface yes", "inf", "-inf surface yes", "1e999", "1e-3x", "x", "1e-3 surface", "1e-3 size",
                        "1e-3 surface maybe", "1e-3 size 1", "1e-3 yes", "1e-3 surface yes size", "1e-3 surface yes extra",
                        "1e-3 1e-3", "1e-3 cutoff 2", "1e-3 Surface yes", "1e-3 surface YES", "'' surface yes", "1e-3 '' yes"})
    cluster_bad(s);
  {
    sf::ClusterSpec S;
    const std::string e = sf::parse_cluster_atom(words("compute cl all cluster/atom"), &S);
    expect(e == "Illegal compute cluster/atom command", "cluster/atom (four words)", e);
  }

  // ---- the bond-based siblings ----
  for (const char* s : {"fragment/atom", "aggregate/atom"}) {
    const std::string e = sf::cluster_unsupported_style(s);
    expect(e == std::string("compute ") + s + " is not supported (there are no bonds; cluster/atom is)", s, e);
  }
  for (const char* s : {"cluster/atom", "cluster/stats", "coord/atom", "fragment", ""})
    expect(sf::cluster_unsupported_style(s).empty(), std::string("style '") + s + "'", sf::cluster_unsupported_style(s));

  // ---- compute cluster/stats ----
  stats_ok("cl", "cl");
  stats_ok("flocs_2", "flocs_2");
  const std::string sbad = "Illegal compute cluster/stats command";
  stats_bad("compute st all cluster/stats", sbad);
  stats_bad("compute st all cluster/stats cl extra", sbad);
  stats_bad("compute st all cluster/stats ''", sbad);
  stats_bad("compute st all cluster/stats cl size yes", sbad);
  stats_bad("compute st all cluster/stats c_cl", "give the ID of the cluster/atom compute itself (cl, not c_cl)");

  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
