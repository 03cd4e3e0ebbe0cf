// histo_parse_check.cpp -- the host-only parser, bins and averager of csrc/sf_histo_parse.h over well- and ill-formed lines, as
// a stand-alone program for the host sanitizers (tests/test_histo_parse.py builds it with -fsanitize=address,undefined and
// runs it once).  Prints one line per case; exit status 0 when every case gave what is expected of it.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_histo_parse.h"

namespace {
int failures = 0;

void expect(bool ok, const std::string& what, const std::string& got)
{
  std::printf("%s %s -> %s\n", ok ? "ok  " : "FAIL", what.c_str(), got.empty() ? "(accepted)" : got.c_str());
  if (!ok) failures++;
}

std::string histo(const std::string& args, sf::HistoSpec* S, const std::string& style = "ave/histo")
{
  std::vector<std::string> w;
  const std::string q = sf::split_quoted("fix h all " + style + " " + args, &w);
  return q.empty() ? sf::parse_ave_histo(w, S) : q;
}

sf::HistoSpec histo_ok(const std::string& args, size_t nvalues)
{
  sf::HistoSpec S;
  const std::string e = histo(args, &S);
  expect(e.empty() && S.values.size() == nvalues, "ave/histo " + args, e);
  return S;
}

void histo_bad(const std::string& args, const std::string& part)
{
  sf::HistoSpec S;
  const std::string e = histo(args, &S);
  expect(!e.empty() && e.find(part) != std::string::npos, "ave/histo " + args, e);
}

void bins_are(int beyond, const std::vector<int>& want, double total, double missing)
{
  const double v[9] = {1, 2, 1, 1, 2, 0.5, 3.0, 1.25, 1.999999};
  const sf::HistoBins B = sf::histo_bins(1.0, 2.0, 4, beyond);
  std::vector<int> got(B.nbins, 0);
  double t = 0, m = 0;
  for (double x : v) {
    const int b = sf::histo_bin(B, x);
    if (b < 0) m++;
    else if (b < B.nbins) got[b]++, t++;
  }
  expect(got == want && t == total && m == missing && B.nbins == (int)want.size(), "hand bins, beyond " + std::to_string(beyond), "");
}
}  // namespace

int main()
{
  const std::string illegal = "Illegal fix ave/histo command";
  // ---- well-formed ----
  {
    sf::HistoSpec S = histo_ok("2 3 10 -1.5 2.5 40 vx vy vz mode vector", 3);
    expect(S.nevery == 2 && S.nrepeat == 3 && S.nfreq == 10 && S.lo == -1.5 && S.hi == 2.5 && S.nbin == 40 && S.mode == sf::HM_VECTOR &&
               S.beyond == sf::HB_IGNORE && S.ave == sf::AVE_ONE && S.kind == sf::HK_NONE && S.values[2].attr == sf::AA_VZ,
           "  its fields", "");
    S = histo_ok("1 1 1 0 1 8192 c_r", 1);
    expect(S.mode == sf::HM_SCALAR && S.values[0].attr == sf::AA_COMPUTE && S.values[0].id == "r" && S.values[0].index == 0, "  its fields", "");
    S = histo_ok("1 1 1 0 1 10 c_s[4] c_k x mode vector kind peratom beyond extra ave window 3 start 20 file out.txt overwrite", 3);
    expect(S.values[0].id == "s" && S.values[0].index == 4 && S.values[0].word == "c_s[4]" && S.kind == sf::HK_PERATOM &&
               S.beyond == sf::HB_EXTRA && S.ave == sf::AVE_WINDOW && S.window == 3 && S.start == 20 && S.file == "out.txt" && S.overwrite,
           "  its fields", "");
    S = histo_ok("5 2 10 0 1 10 c_pl[2] mode vector kind local beyond end ave running", 1);
    expect(S.kind == sf::HK_LOCAL && S.beyond == sf::HB_END && S.ave == sf::AVE_RUNNING, "  its fields", "");
    S = histo_ok("1 1 1 0 1 10 c_r kind global mode scalar ave one beyond ignore", 1);
    expect(S.kind == sf::HK_GLOBAL && S.mode == sf::HM_SCALAR, "  its fields", "");
    // quoted titles
    S = histo_ok("1 1 1 0 1 10 vx mode vector title1 \"# one two\" title2 '# three  four' title3 \"# it's\" file f", 1);
    expect(S.has_title[0] && S.has_title[1] && S.has_title[2] && S.title[0] == "# one two" && S.title[1] == "# three  four" &&
               S.title[2] == "# it's" && S.file == "f",
           "  its titles", "");
    S = histo_ok("1 1 1 0 1 10 vx mode vector title1 \"\"", 1);
    expect(S.has_title[0] && S.title[0].empty() && !S.has_title[1], "  an empty title", "");
    // each keyword twice: the last one holds
    S = histo_ok("1 1 1 0 1 10 vx mode scalar mode vector kind global kind peratom beyond end beyond extra ave running ave window 2 "
                 "ave one start 5 start 7 file a file b overwrite overwrite title1 a title1 b title2 a title2 b title3 a title3 b",
                 1);
    expect(S.mode == sf::HM_VECTOR && S.kind == sf::HK_PERATOM && S.beyond == sf::HB_EXTRA && S.ave == sf::AVE_ONE && S.start == 7 &&
               S.file == "b" && S.overwrite && S.title[0] == "b" && S.title[1] == "b" && S.title[2] == "b",
           "  the last of each keyword", "");
    histo_ok("1 1 1 0 1 10 x y z vx vy vz fx fy fz c_a c_b c_c c_d c_e c_f c_g mode vector", 16);
    histo_ok("10 10 100 1e-3 1e3 100 fx   # a comment", 1);
  }
  // ---- ill-formed ----
  histo_bad("", illegal);
  histo_bad("1 1 1 0 1 10", illegal);                 // no value
  histo_bad("1 1 1 0 1 10 mode vector", illegal);     // no value
  histo_bad("0 1 1 0 1 10 vx", illegal);
  histo_bad("1 0 1 0 1 10 vx", illegal);
  histo_bad("1 1 0 0 1 10 vx", illegal);
  histo_bad("-1 1 1 0 1 10 vx", illegal);
  histo_bad("3 3 10 0 1 10 vx", illegal);             // Nfreq is no multiple of Nevery
  histo_bad("2 6 10 0 1 10 vx", illegal);             // Nrepeat * Nevery > Nfreq
  histo_bad("a 1 1 0 1 10 vx", illegal);
  histo_bad("1 1 1 1 1 10 vx", illegal);              // lo == hi
  histo_bad("1 1 1 2 1 10 vx", illegal);              // lo > hi
  histo_bad("1 1 1 x 1 10 vx", illegal);
  histo_bad("1 1 1 0 nan 10 vx", illegal);
  histo_bad("1 1 1 0 inf 10 vx", illegal);
  histo_bad("1 1 1 0 1 0 vx", illegal);               // Nbin 0
  histo_bad("1 1 1 0 1 -4 vx", illegal);
  histo_bad("1 1 1 0 1 2.5 vx", illegal);
  histo_bad("1 1 1 0 1 8193 vx", "more than 8192 bins");
  histo_bad("1 1 1 0 1 10 vx bogus", illegal);        // an unknown keyword
  histo_bad("1 1 1 0 1 10 vx omegax", illegal);
  histo_bad("1 1 1 0 1 10 vx vy mode", illegal);      // keywords cut short
  histo_bad("1 1 1 0 1 10 vx kind", illegal);
  histo_bad("1 1 1 0 1 10 vx beyond", illegal);
  histo_bad("1 1 1 0 1 10 vx ave", illegal);
  histo_bad("1 1 1 0 1 10 vx ave window", illegal);
  histo_bad("1 1 1 0 1 10 vx start", illegal);
  histo_bad("1 1 1 0 1 10 vx file", illegal);
  histo_bad("1 1 1 0 1 10 vx title1", illegal);
  histo_bad("1 1 1 0 1 10 vx title2", illegal);
  histo_bad("1 1 1 0 1 10 vx title3", illegal);
  histo_bad("1 1 1 0 1 10 vx mode matrix", illegal);
  histo_bad("1 1 1 0 1 10 vx kind atom", illegal);
  histo_bad("1 1 1 0 1 10 vx beyond both", illegal);
  histo_bad("1 1 1 0 1 10 vx ave sometimes", illegal);
  histo_bad("1 1 1 0 1 10 vx ave window 0", illegal);
  histo_bad("1 1 1 0 1 10 vx ave window x", illegal);
  histo_bad("1 1 1 0 1 10 vx start -1", illegal);
  histo_bad("1 1 1 0 1 10 vx file \"\"", illegal);
  histo_bad("1 1 1 0 1 10 c_", illegal);
  histo_bad("1 1 1 0 1 10 c_k[", illegal);
  histo_bad("1 1 1 0 1 10 c_k[0]", illegal);
  histo_bad("1 1 1 0 1 10 c_k[1]x", illegal);
  histo_bad("1 1 1 0 1 10 c_k[-1]", illegal);
  histo_bad("1 1 1 0 1 10 c_k[*]", "c_k[*] is not supported");
  histo_bad("1 1 1 0 1 10 f_a", "f_a is not supported");
  histo_bad("1 1 1 0 1 10 v_a", "v_a is not supported");
  histo_bad("1 1 1 0 1 10 vx append out.txt", "append is not supported");
  histo_bad("1 1 1 0 1 10 vx title1 \"# open", "Unbalanced quotes");
  histo_bad("1 1 1 0 1 10 x y z vx vy vz fx fy fz c_a c_b c_c c_d c_e c_f c_g c_h", "more than 16 values");
  {
    sf::HistoSpec S;
    const std::string e = histo("1 1 1 0 1 10 vx vy", &S, "ave/histo/weight");
    expect(e.find("fix ave/histo/weight is not supported") == 0 && e.find("sort-and-segment") != std::string::npos, "ave/histo/weight", e);
  }
  // ---- the bins ----
  bins_are(sf::HB_IGNORE, {3, 1, 0, 3}, 7, 2);
  bins_are(sf::HB_END, {4, 1, 0, 4}, 9, 0);
  bins_are(sf::HB_EXTRA, {1, 3, 1, 0, 1, 3}, 9, 0);
  {
    const sf::HistoBins B = sf::histo_bins(1.0, 2.0, 4, sf::HB_EXTRA), P = sf::histo_bins(1.0, 2.0, 4, sf::HB_IGNORE);
    expect(B.nbins == 6 && B.bininv == 4.0 && sf::histo_coord(B, 0) == 1.0 && sf::histo_coord(B, 1) == 1.125 && sf::histo_coord(B, 4) == 1.875 &&
               sf::histo_coord(B, 5) == 2.0 && sf::histo_coord(P, 0) == 1.125 && sf::histo_coord(P, 3) == 1.875,
           "coordinates", "");
    // whatever the value, the bin is in range
    const double odd[8] = {std::numeric_limits<double>::quiet_NaN(), -std::numeric_limits<double>::quiet_NaN(),
                           std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), 1.0e300, -1.0e300,
                           std::nextafter(2.0, 3.0), std::nextafter(1.0, 0.0)};
    bool in_range = true;
    for (int beyond = 0; beyond < 3; beyond++) {
      const sf::HistoBins Q = sf::histo_bins(1.0, 2.0, 4, beyond);
      for (double x : odd) {
        const int b = sf::histo_bin(Q, x);
        if (b < -1 || b >= Q.nbins || (b == -1 && beyond != sf::HB_IGNORE)) in_range = false;
      }
    }
    expect(in_range, "odd values stay in range", "");
    const sf::HistoBins W = sf::histo_bins(-1.0e300, 1.0e300, 8192, sf::HB_END);
    expect(sf::histo_bin(W, 1.0e300) == 8191 && sf::histo_bin(W, -1.0e300) == 0 && sf::histo_bin(W, 0.0) >= 4095 && sf::histo_bin(W, 0.0) <= 4096, "a wide range", "");
  }
  // ---- the averager ----
  {
    auto block = [](std::vector<double> c, double total, double missing, double mn, double mx) {
      sf::HistoBlock b;
      b.count = c;
      b.total = total;
      b.missing = missing;
      b.min = mn;
      b.max = mx;
      return b;
    };
    const sf::HistoBlock b[4] = {block({1, 1, 0, 0}, 2, 0, 0.5, 1.5), block({0, 0, 1, 0}, 1, 1, 2.5, 9.0),
                                 block({0, 0, 0, 2}, 2, 1, -1.0, 3.5), block({1, 0, 0, 0}, 1, 0, 0.5, 0.5)};
    sf::HistoAverager one, run, win;
    run.ave = sf::AVE_RUNNING;
    win.ave = sf::AVE_WINDOW;
    win.window = 2;
    sf::HistoBlock o, r, w;
    for (int k = 0; k < 4; k++) o = one.add(b[k]), r = run.add(b[k]), w = win.add(b[k]);
    expect(o.count == std::vector<double>({1, 0, 0, 0}) && o.total == 1 && o.min == 0.5 && o.max == 0.5, "ave one", "");
    expect(r.count == std::vector<double>({2, 1, 1, 2}) && r.total == 6 && r.missing == 2 && r.min == -1.0 && r.max == 9.0, "ave running", "");
    expect(w.count == std::vector<double>({1, 0, 0, 2}) && w.total == 3 && w.missing == 1 && w.min == -1.0 && w.max == 3.5, "ave window 2", "");
    sf::HistoBlock empty;
    empty.count.assign(4, 0.0);
    sf::HistoAverager e;
    const sf::HistoBlock q = e.add(empty);
    expect(q.total == 0 && q.min == 1.0e20 && q.max == -1.0e20, "an empty block", "");
  }
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
