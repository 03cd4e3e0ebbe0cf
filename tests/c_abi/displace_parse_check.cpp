// displace_parse_check.cpp -- the host-only parsers of csrc/sf_displace_parse.h and the attribute names xu yu zu ix iy iz of
// csrc/sf_global_parse.h over well- and ill-formed lines, as a stand-alone program for the host sanitizers
// (tests/test_displace_parse.py builds it with -fsanitize=address,undefined and runs it once).  Prints one line per case;
// exit status 0 when every case gave what is expected of it.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_displace_parse.h"
#include "../../sedifoam_amd/csrc/sf_global_parse.h"

namespace {
int failures = 0;

void expect(bool ok, const std::string& what, const std::string& got)
{
  std::printf("%s %s -> %s\n", ok ? "ok  " : "FAIL", what.c_str(), got.empty() ? "(accepted)" : got.c_str());
  if (!ok) failures++;
}

std::vector<std::string> words(const std::string& line, std::string* err)
{
  std::vector<std::string> w;
  *err = sf::split_quoted(line, &w);
  return w;
}
}  // namespace

int main()
{
  // ---- compute property/atom: the new names ----
  {
    std::string e;
    std::vector<int> a;
    std::vector<std::string> w = words("compute p all property/atom xu yu zu ix iy iz", &e);
    if (e.empty()) e = sf::parse_property_atom(w, &a);
    const int want[6] = {sf::PA_XU, sf::PA_YU, sf::PA_ZU, sf::PA_IX, sf::PA_IY, sf::PA_IZ};
    bool same = a.size() == 6;
    for (size_t k = 0; same && k < 6; k++) same = a[k] == want[k] && sf::prop_attr_needs_image(a[k]);
    expect(e.empty() && same, "property/atom xu yu zu ix iy iz", e);
    w = words("compute p all property/atom x ix id", &e);
    if (e.empty()) e = sf::parse_property_atom(w, &a);
    expect(e.empty() && a.size() == 3 && a[0] == sf::PA_X && a[1] == sf::PA_IX && a[2] == sf::PA_ID &&
               !sf::prop_attr_needs_image(a[0]) && !sf::prop_attr_needs_image(a[2]),
           "property/atom x ix id", e);
    for (const char* bad : {"xs", "xsu", "iw", "xu[1]", "XU", "image"}) {
      w = words(std::string("compute p all property/atom ") + bad, &e);
      if (e.empty()) e = sf::parse_property_atom(w, &a);
      expect(e == std::string("Invalid keyword in compute property/atom command: ") + bad, std::string("property/atom ") + bad, e);
    }
    for (int q = 0; q < sf::PA_COUNT_ALL; q++) {   // every name is its own attribute, and nothing lies beyond the table
      w = words(std::string("compute p all property/atom ") + sf::prop_attr_name(q), &e);
      if (e.empty()) e = sf::parse_property_atom(w, &a);
      expect(e.empty() && a.size() == 1 && a[0] == q, std::string("property/atom ") + sf::prop_attr_name(q), e);
    }
    expect(std::string(sf::prop_attr_name(sf::PA_COUNT_ALL)).empty() && std::string(sf::prop_attr_name(-1)).empty(),
           "prop_attr_name out of range", "");
  }
  // ---- compute displace/atom, compute com ----
  {
    std::string e;
    std::vector<std::string> w = words("compute d all displace/atom", &e);
    if (e.empty()) e = sf::parse_displace_atom(w);
    expect(e.empty(), "displace/atom", e);
    w = words("compute d all displace/atom extra", &e);
    if (e.empty()) e = sf::parse_displace_atom(w);
    expect(e == "Illegal compute displace/atom command", "displace/atom extra", e);
    w = words("compute d all displace/atom refresh v", &e);
    if (e.empty()) e = sf::parse_displace_atom(w);
    expect(e == "Illegal compute displace/atom command", "displace/atom refresh v", e);
    w = words("compute c all com", &e);
    if (e.empty()) e = sf::parse_com(w);
    expect(e.empty(), "com", e);
    w = words("compute c all com extra", &e);
    if (e.empty()) e = sf::parse_com(w);
    expect(e == "Illegal compute com command", "com extra", e);
    w = words("compute c all com 'extra", &e);
    expect(e == "Unbalanced quotes in input line", "com 'extra", e);
    expect(sf::parse_com({"compute", "c"}) == "Illegal compute com command", "com (two words)", "");
    expect(sf::parse_displace_atom({}) == "Illegal compute displace/atom command", "displace/atom (no words)", "");
  }
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
