// global_parse_check.cpp -- the host-only parsers of csrc/sf_global_parse.h over well- and ill-formed lines, as a stand-alone
// program for the host sanitizers (tests/test_global_parse.py builds it with -fsanitize=address,undefined and runs it once).
// Prints one line per case; exit status 0 when every case gave what is expected of it.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_global_parse.h"

namespace {
int failures = 0;

void expect(bool ok, const std::string& what, const std::string& got)
{
  std::printf("%s %s -> %s\n", ok ? "ok  " : "FAIL", what.c_str(), got.empty() ? "(accepted)" : got.c_str());
  if (!ok) failures++;
}

std::string reduce(const std::string& args, sf::ReduceSpec* S)
{
  std::vector<std::string> w;
  const std::string q = sf::split_quoted("compute r all reduce " + args, &w);
  return q.empty() ? sf::parse_reduce(w, S) : q;
}

void reduce_ok(const std::string& args, int mode, size_t ninputs)
{
  sf::ReduceSpec S;
  const std::string e = reduce(args, &S);
  expect(e.empty() && S.mode == mode && S.inputs.size() == ninputs, "reduce " + args, e);
}

void reduce_bad(const std::string& args, const std::string& part)
{
  sf::ReduceSpec S;
  const std::string e = reduce(args, &S);
  expect(!e.empty() && e.find(part) != std::string::npos, "reduce " + args, e);
}

std::string prop(const std::string& args, std::vector<int>* a)
{
  std::vector<std::string> w;
  const std::string q = sf::split_quoted("compute p all property/atom " + args, &w);
  return q.empty() ? sf::parse_property_atom(w, a) : q;
}

std::string avet(const std::string& args, sf::AveTimeSpec* S)
{
  std::vector<std::string> w;
  const std::string q = sf::split_quoted("fix t all ave/time " + args, &w);
  return q.empty() ? sf::parse_ave_time(w, S) : q;
}

void avet_ok(const std::string& args, size_t nvalues)
{
  sf::AveTimeSpec S;
  const std::string e = avet(args, &S);
  expect(e.empty() && S.values.size() == nvalues, "ave/time " + args, e);
}

void avet_bad(const std::string& args, const std::string& part)
{
  sf::AveTimeSpec S;
  const std::string e = avet(args, &S);
  expect(!e.empty() && e.find(part) != std::string::npos, "ave/time " + args, e);
}

void thermo_ok(const std::string& word, const std::string& id, long index)
{
  std::string got;
  long k = -1;
  const std::string e = sf::parse_thermo_column(word, &got, &k);
  expect(e.empty() && got == id && k == index, "thermo " + word, e);
}

void thermo_bad(const std::string& word)
{
  std::string got;
  long k = -1;
  const std::string e = sf::parse_thermo_column(word, &got, &k);
  expect(e.find("Invalid keyword in thermo_style custom command") == 0, "thermo " + word, e);
}
}  // namespace

int main()
{
  const std::string illegal = "Illegal compute reduce command";
  // ---- compute reduce ----
  reduce_ok("sum vx", sf::GM_SUM, 1);
  reduce_ok("min x y z", sf::GM_MIN, 3);
  reduce_ok("max y", sf::GM_MAX, 1);
  reduce_ok("ave c_k", sf::GM_AVE, 1);
  reduce_ok("sumsq c_s[4] fx", sf::GM_SUMSQ, 2);
  reduce_ok("avesq vx vy vz fx fy fz c_a c_b[1] c_b[1000000]", sf::GM_AVESQ, 9);
  reduce_ok("sum vx   # a comment", sf::GM_SUM, 1);
  {
    sf::ReduceSpec S;
    const std::string e = reduce("sum c_st[6] vy", &S);
    expect(e.empty() && S.inputs[0].attr == sf::AA_COMPUTE && S.inputs[0].id == "st" && S.inputs[0].index == 6 &&
               S.inputs[0].word == "c_st[6]" && S.inputs[1].attr == sf::AA_VY && S.id == "r" && S.group == "all",
           "reduce sum c_st[6] vy (fields)", e);
  }
  reduce_bad("", illegal);
  reduce_bad("sum", illegal);
  reduce_bad("total vx", illegal);
  reduce_bad("sum vx vw", illegal);
  reduce_bad("sum c_", illegal);
  reduce_bad("sum c_a[", illegal);
  reduce_bad("sum c_a[]", illegal);
  reduce_bad("sum c_a[0]", illegal);
  reduce_bad("sum c_a[-1]", illegal);
  reduce_bad("sum c_a[ 1]", illegal);
  reduce_bad("sum c_a[1", illegal);
  reduce_bad("sum c_a[1]x", illegal);
  reduce_bad("sum c_a]1[", illegal);
  reduce_bad("sum c_[1]", illegal);
  reduce_bad("sum c_a[1.5]", illegal);
  reduce_bad("sum c_a[nan]", illegal);
  reduce_bad("sum c_a[99999999999999999999999999]", illegal);
  reduce_bad("sum c_a[1000001]", illegal);
  reduce_bad("sumabs vx", "sumabs is not supported");
  reduce_bad("aveabs vx", "aveabs is not supported");
  reduce_bad("minabs vx", "not supported");
  reduce_bad("maxabs vx", "not supported");
  reduce_bad("sum vx replace 1 2", "replace is not supported");
  reduce_bad("sum vx inputs peratom", "inputs is not supported");
  reduce_bad("sum f_1", "f_1 is not supported");
  reduce_bad("sum vx v_a", "v_a is not supported");
  reduce_bad("sum 'vx", "Unbalanced quotes");
  {
    std::string many = "sum";
    for (int k = 0; k < 65; k++) many += " vx";
    reduce_bad(many, "more than 64 inputs");
  }
  // ---- compute property/atom ----
  {
    std::vector<int> a;
    std::string e = prop("id type mass radius diameter x y z vx vy vz fx fy fz omegax omegay omegaz tqx tqy tqz", &a);
    bool in_order = a.size() == (size_t)sf::PA_COUNT;
    for (size_t k = 0; in_order && k < a.size(); k++) in_order = a[k] == (int)k;
    expect(e.empty() && in_order, "property/atom (every attribute)", e);
    e = prop("radius", &a);
    expect(e.empty() && a.size() == 1 && a[0] == sf::PA_RADIUS, "property/atom radius", e);
    e = prop("", &a);
    expect(e == "Illegal compute property/atom command", "property/atom (nothing)", e);
    e = prop("radius q", &a);
    expect(e == "Invalid keyword in compute property/atom command: q", "property/atom radius q", e);
    e = prop("mol", &a);
    expect(e.find("Invalid keyword") == 0, "property/atom mol", e);
    e = prop("x x x x x x x x x x x x x x x x x x x x x x x x x", &a);
    expect(e.find("more than 24") != std::string::npos, "property/atom (25 attributes)", e);
    e = prop("\"x", &a);
    expect(e == "Unbalanced quotes in input line", "property/atom \"x", e);
  }
  // ---- fix ave/time ----
  const std::string bad = "Illegal fix ave/time command";
  avet_ok("2 3 10 c_r", 1);
  avet_ok("10 1 10 c_r c_v[2] c_v[1]", 3);
  avet_ok("5 2 10 c_r start 25 ave running file out.txt overwrite", 1);
  avet_ok("5 2 10 c_r ave window 2 mode scalar title3 unused", 1);
  avet_ok("5 2 10 c_r format %.10g", 1);
  avet_ok("5 2 10 c_r format \" %14.6e\" title1 \"# one two\" title2 '# three four'", 1);
  {
    sf::AveTimeSpec S;
    const std::string e = avet("5 2 10 c_a c_b[3] ave window 7 start 25 file f.txt title1 \"# a b\" format \" %.3f\"", &S);
    expect(e.empty() && S.nevery == 5 && S.nrepeat == 2 && S.nfreq == 10 && S.ave == sf::AVE_WINDOW && S.window == 7 &&
               S.start == 25 && S.file == "f.txt" && S.has_title[0] && S.title[0] == "# a b" && !S.has_title[1] &&
               S.format == " %.3f" && S.values[1].id == "b" && S.values[1].index == 3 && S.values[1].word == "c_b[3]" &&
               !S.overwrite,
           "ave/time (fields)", e);
    sf::AveTimeSpec D;
    const std::string d = avet("1 1 1 c_a", &D);
    expect(d.empty() && D.format == " %g" && D.ave == sf::AVE_ONE && D.start == 0 && D.file.empty(), "ave/time (defaults)", d);
  }
  avet_bad("", bad);
  avet_bad("2 3", bad);
  avet_bad("2 3 10", bad);
  avet_bad("0 3 10 c_r", bad);
  avet_bad("2 0 10 c_r", bad);
  avet_bad("2 3 0 c_r", bad);
  avet_bad("-2 3 10 c_r", bad);
  avet_bad("3 3 10 c_r", bad);            // Nfreq % Nevery
  avet_bad("2 6 10 c_r", bad);            // Nrepeat * Nevery > Nfreq
  avet_bad("2 3 ten c_r", bad);
  avet_bad("2 3 1e1 c_r", bad);
  avet_bad("2 3 nan c_r", bad);
  avet_bad("99999999999999999999 1 99999999999999999999 c_r", bad);
  avet_bad("2 3 10 vx", bad);
  avet_bad("2 3 10 c_", bad);
  avet_bad("2 3 10 c_a[", bad);
  avet_bad("2 3 10 c_a[0]", bad);
  avet_bad("2 3 10 c_a[2", bad);
  avet_bad("2 3 10 c_r ave", bad);
  avet_bad("2 3 10 c_r ave sometimes", bad);
  avet_bad("2 3 10 c_r ave window", bad);
  avet_bad("2 3 10 c_r ave window 0", bad);
  avet_bad("2 3 10 c_r ave window nan", bad);
  avet_bad("2 3 10 c_r ave window 99999999999999999999", bad);
  avet_bad("2 3 10 c_r start", bad);
  avet_bad("2 3 10 c_r start -5", bad);
  avet_bad("2 3 10 c_r start 99999999999999999999", bad);
  avet_bad("2 3 10 c_r file", bad);
  avet_bad("2 3 10 c_r title1", bad);
  avet_bad("2 3 10 c_r format", bad);
  avet_bad("2 3 10 c_r mode", bad);
  avet_bad("2 3 10 c_r colour red", bad);
  avet_bad("2 3 10 c_r format %s", "is not one %g-class conversion");
  avet_bad("2 3 10 c_r format %g%g", "is not one %g-class conversion");
  avet_bad("2 3 10 c_r format %d", "is not one %g-class conversion");
  avet_bad("2 3 10 c_r format %n", "is not one %g-class conversion");
  avet_bad("2 3 10 c_r format \"%g \"", "is not one %g-class conversion");
  avet_bad("2 3 10 c_r format %9999g", "is not one %g-class conversion");
  avet_bad("2 3 10 c_r mode vector", "mode vector is not supported");
  avet_bad("2 3 10 c_r off 1", "off is not supported");
  avet_bad("2 3 10 f_1", "f_1 is not supported");
  avet_bad("2 3 10 c_r v_x", "v_x is not supported");
  avet_bad("2 3 10 c_r title1 \"# no end", "Unbalanced quotes");
  avet_bad("2 3 10 c_r title2 '# no end", "Unbalanced quotes");
  {
    std::string many = "1 1 1";
    for (int k = 0; k < 65; k++) many += " c_r";
    avet_bad(many, "more than 64 values");
  }
  // ---- the schedule ----
  {
    const long long a = sf::ave_first_valid(0, 2, 3, 10), b = sf::ave_first_valid(7, 2, 3, 10), c = sf::ave_first_valid(0, 10, 1, 10),
                    d = sf::ave_first_valid(7, 10, 1, 10), e = sf::ave_first_valid(0, 5, 2, 10, 25), f = sf::ave_first_valid(30, 5, 2, 10, 25),
                    g = sf::ave_first_valid(0, 5, 2, 10, 10);
    expect(a == 6 && b == 16 && c == 0 && d == 10 && e == 25 && f == 35 && g == 5, "ave_first_valid",
           std::to_string(a) + " " + std::to_string(b) + " " + std::to_string(c) + " " + std::to_string(d) + " " +
               std::to_string(e) + " " + std::to_string(f) + " " + std::to_string(g));
  }
  // ---- thermo_style custom ... c_ ----
  thermo_ok("c_r", "r", 0);
  thermo_ok("c_r2[2]", "r2", 2);
  thermo_ok("c_a_b[10]", "a_b", 10);
  thermo_bad("c_");
  thermo_bad("c_a[");
  thermo_bad("c_a[0]");
  thermo_bad("c_a[]");
  thermo_bad("c_a[1]]");
  thermo_bad("c_a[+1]");
  thermo_bad("c_[2]");
  thermo_bad("c_a[99999999999999999999]");
  thermo_bad("c_a[nan]");
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
