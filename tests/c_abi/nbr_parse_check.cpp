// nbr_parse_check.cpp -- the host-only parsers of csrc/sf_nbr_parse.h and the mode-vector words of csrc/sf_global_parse.h over
// well- and ill-formed lines, as a stand-alone program for the host sanitizers (tests/test_nbr_parse.py builds it with
// -fsanitize=address,undefined and runs it once).  Prints one line per case; exit status 0 when every case gave what is
// expected of it.
#include <climits>
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

void range_ok(const std::string& s, int lo, int hi)
{
  sf::TypeRange r;
  const bool ok = sf::parse_type_range(s, &r);
  expect(ok && r.lo == lo && r.hi == hi, "range " + s, ok ? "" : "refused");
}

void range_bad(const std::string& s)
{
  sf::TypeRange r;
  expect(!sf::parse_type_range(s, &r), "range '" + s + "'", "refused");
}

void rdf_ok(const std::string& args, long nbin, size_t npairs, double rc)
{
  sf::RdfSpec S;
  const std::string e = sf::parse_rdf(words("compute g all rdf " + args), &S);
  expect(e.empty() && S.nbin == nbin && S.pairs.size() == npairs && S.rc == rc, "rdf " + args, e);
}

void rdf_bad(const std::string& args, const std::string& part)
{
  sf::RdfSpec S;
  const std::string e = sf::parse_rdf(words("compute g all rdf " + args), &S);
  expect(!e.empty() && e.find(part) != std::string::npos, "rdf " + args, e);
}

void coord_ok(const std::string& args, size_t nranges, double rc)
{
  sf::CoordSpec S;
  const std::string e = sf::parse_coord_atom(words("compute c all coord/atom " + args), &S);
  expect(e.empty() && S.ranges.size() == nranges && S.rc == rc, "coord/atom " + args, e);
}

void coord_bad(const std::string& args, const std::string& part)
{
  sf::CoordSpec S;
  const std::string e = sf::parse_coord_atom(words("compute c all coord/atom " + args), &S);
  expect(!e.empty() && e.find(part) != std::string::npos, "coord/atom " + args, e);
}

void avet_ok(const std::string& args, size_t nvalues, bool vector)
{
  sf::AveTimeSpec S;
  const std::string e = sf::parse_ave_time(words("fix t all ave/time " + args), &S);
  expect(e.empty() && S.values.size() == nvalues && S.mode_vector == vector, "ave/time " + args, e);
}

void avet_bad(const std::string& args, const std::string& part)
{
  sf::AveTimeSpec S;
  const std::string e = sf::parse_ave_time(words("fix t all ave/time " + args), &S);
  expect(!e.empty() && e.find(part) != std::string::npos, "ave/time " + args, e);
}
}  // namespace

int main()
{
  // ---- a type range ----
  range_ok("1", 1, 1);
  range_ok("12", 12, 12);
  range_ok("1*2", 1, 2);
  range_ok("3*3", 3, 3);
  range_ok("2*", 2, INT_MAX);
  range_ok("*2", INT_MIN, 2);
  range_ok("*", INT_MIN, INT_MAX);
  for (const char* s : {"", "a", "-1", "+1", "1.0", "2*1", "1**2", "**", "1*2*3", "1*b", "a*", " 1", "99999999999"}) range_bad(s);

  // ---- compute rdf ----
  rdf_ok("100 cutoff 0.003", 100, 1, 0.003);
  rdf_ok("1 cutoff 1", 1, 1, 1.0);
  rdf_ok("7 * * cutoff 2.5e-3", 7, 1, 2.5e-3);
  rdf_ok("7 1 1 1 2 2 2 cutoff 0.5", 7, 3, 0.5);
  rdf_ok("7 1*2 2 cutoff 0.5", 7, 1, 0.5);
  rdf_ok("7 1* *2 cutoff 0.5", 7, 1, 0.5);
  rdf_ok("8192 cutoff 0.5", 8192, 1, 0.5);
  rdf_ok("4096 1 1 2 2 cutoff 0.5", 4096, 2, 0.5);
  {
    sf::RdfSpec S;
    const std::string e = sf::parse_rdf(words("compute g all rdf 5 1*2 2 3 * cutoff 0.25"), &S);
    expect(e.empty() && S.pairs.size() == 2 && S.pairs[0].i.lo == 1 && S.pairs[0].i.hi == 2 && S.pairs[0].j.lo == 2 &&
               S.pairs[0].j.hi == 2 && S.pairs[1].i.lo == 3 && S.pairs[1].j.lo == INT_MIN && S.pairs[1].j.hi == INT_MAX &&
               S.id == "g" && S.group == "all",
           "rdf 5 1*2 2 3 * cutoff 0.25 (the ranges)", e);
  }
  const std::string bad = "Illegal compute rdf command";
  rdf_bad("", bad);
  rdf_bad("0 cutoff 1", bad);
  rdf_bad("-3 cutoff 1", bad);
  rdf_bad("ten cutoff 1", bad);
  rdf_bad("1.5 cutoff 1", bad);
  rdf_bad("10 1 cutoff 1", bad);
  rdf_bad("10 1 1 2 cutoff 1", bad);
  rdf_bad("10 1 x cutoff 1", bad);
  rdf_bad("10 2*1 1 cutoff 1", bad);
  rdf_bad("10 cutoff", bad);
  rdf_bad("10 cutoff 0", bad);
  rdf_bad("10 cutoff -1", bad);
  rdf_bad("10 cutoff 1x", bad);
  rdf_bad("10 cutoff nan", bad);
  rdf_bad("10 cutoff inf", bad);
  rdf_bad("10 cutoff 1 extra", bad);
  rdf_bad("10 cutoff 1 cutoff 2", bad);
  rdf_bad("10", "the cutoff keyword is required");
  rdf_bad("10 1 1", "the cutoff keyword is required");
  rdf_bad("10 1 1 2 2", "the cutoff keyword is required");
  rdf_bad("8193 cutoff 1", "above 8192");
  rdf_bad("4097 1 1 2 2 cutoff 1", "above 8192");
  rdf_bad("1999999999 1 1 2 2 3 3 cutoff 1", "above 8192");

  // ---- compute coord/atom ----
  coord_ok("cutoff 0.003", 1, 0.003);
  coord_ok("cutoff 2 *", 1, 2.0);
  coord_ok("cutoff 2 1", 1, 2.0);
  coord_ok("cutoff 2 1 2 1*2", 3, 2.0);
  coord_ok("cutoff 2 1 2 3 4 5 6 7 8", 8, 2.0);
  const std::string cbad = "Illegal compute coord/atom command";
  coord_bad("", cbad);
  coord_bad("cutoff", cbad);
  coord_bad("cutoff 0", cbad);
  coord_bad("cutoff -2", cbad);
  coord_bad("cutoff two", cbad);
  coord_bad("cutoff 2 x", cbad);
  coord_bad("cutoff 2 2*1", cbad);
  coord_bad("cutoff 2 1 2 3 4 5 6 7 8 9", "more than 8 type ranges");
  coord_bad("orientorder o 0.5", "only cstyle cutoff is supported");
  coord_bad("2.0", "only cstyle cutoff is supported");
  coord_bad("2.0 1 2", "only cstyle cutoff is supported");

  // ---- fix ave/time mode vector ----
  avet_ok("2 3 10 c_g[2] mode vector", 1, true);
  avet_ok("2 3 10 c_g[1] c_g[2] c_h[3] mode vector ave window 2 start 20", 3, true);
  avet_ok("10 1 10 c_g[2] mode vector file f.txt overwrite title3 '# Row g' format ' %.10g'", 1, true);
  avet_ok("2 3 10 c_g[2] mode scalar", 1, false);
  avet_ok("2 3 10 c_g[2]", 1, false);
  {
    sf::AveTimeSpec S;
    const std::string e = sf::parse_ave_time(words("fix t all ave/time 2 3 10 c_g[2] c_h[5] mode vector"), &S);
    expect(e.empty() && sf::ave_time_title3(S) == "# Row c_g[2] c_h[5]", "ave/time title3 of mode vector", e);
  }
  avet_bad("2 3 10 c_r mode vector", "mode vector is not supported");
  avet_bad("2 3 10 c_g[2] c_r mode vector", "mode vector is not supported");
  avet_bad("2 3 10 c_g[2] mode", "Illegal fix ave/time command");
  avet_bad("2 3 10 c_g[2] mode array", "Illegal fix ave/time command");
  avet_bad("2 3 10 c_g[2] mode vector off 1", "off is not supported");
  avet_bad("2 3 10 c_g[0] mode vector", "Illegal fix ave/time command");

  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
