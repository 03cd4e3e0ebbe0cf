// chunk_parse_check.cpp -- the host-only parsers of csrc/sf_chunk_parse.h over well- and ill-formed lines, as a stand-alone
// program for the host sanitizers (tests/test_chunk_parse.py builds it with -fsanitize=address,undefined and runs it once).
// Prints one line per case; exit status 0 when every case gave what is expected of it.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_chunk_parse.h"

namespace {
int failures = 0;

void expect(bool ok, const std::string& what, const std::string& got)
{
  std::printf("%s %s -> %s\n", ok ? "ok  " : "FAIL", what.c_str(), got.empty() ? "(accepted)" : got.c_str());
  if (!ok) failures++;
}

std::string chunk(const std::string& args, sf::ChunkBins* B)
{
  std::vector<std::string> w;
  const std::string q = sf::split_quoted("compute c all chunk/atom " + args, &w);
  if (!q.empty()) return q;
  const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 1.0, 2.0};
  const int per[3] = {1, 0, 1};
  return sf::parse_chunk_atom(w, lo, hi, per, B);
}

std::string ave(const std::string& args, sf::AveSpec* S)
{
  std::vector<std::string> w;
  const std::string q = sf::split_quoted("fix p all ave/chunk " + args, &w);
  if (!q.empty()) return q;
  return sf::parse_ave_chunk(w, S);
}

void chunk_ok(const std::string& args, int nchunk)
{
  sf::ChunkBins B;
  const std::string e = chunk(args, &B);
  expect(e.empty() && B.nchunk == nchunk, "chunk/atom " + args, e.empty() ? "nchunk " + std::to_string(B.nchunk) : e);
}

void chunk_bad(const std::string& args, const std::string& part)
{
  sf::ChunkBins B;
  const std::string e = chunk(args, &B);
  expect(!e.empty() && e.find(part) != std::string::npos, "chunk/atom " + args, e);
}

void ave_ok(const std::string& args, size_t nvalues)
{
  sf::AveSpec S;
  const std::string e = ave(args, &S);
  expect(e.empty() && S.values.size() == nvalues, "ave/chunk " + args, e);
}

void ave_bad(const std::string& args, const std::string& part)
{
  sf::AveSpec S;
  const std::string e = ave(args, &S);
  expect(!e.empty() && e.find(part) != std::string::npos, "ave/chunk " + args, e);
}
}  // namespace

int main()
{
  chunk_ok("bin/1d x lower 0.3 units box", 4);
  chunk_ok("bin/1d x upper 0.3 units box", 4);
  chunk_ok("bin/1d x center 0.3 units box", 4);
  chunk_ok("bin/1d x 0.05 0.3 units box", 5);
  chunk_ok("bin/1d z lower 0.25 units reduced", 4);
  chunk_ok("bin/2d y lower 0.5 x lower 0.25 units box", 8);
  chunk_ok("bin/3d x lower 0.5 y lower 0.5 z lower 0.5 units box discard no nchunk once ids every limit 0 compress no pbc no", 16);
  chunk_ok("bin/1d y lower 0.25 units box bound y 0.25 0.75 discard yes", 2);
  chunk_ok("bin/1d y lower 0.25 bound y lower upper units box # a comment", 4);
  chunk_bad("", "Illegal compute chunk/atom");
  chunk_bad("bin/1d", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower", "Illegal compute chunk/atom");
  chunk_bad("bin/2d x lower 0.5 units box", "Illegal compute chunk/atom");
  chunk_bad("bin/2d x lower 0.5 x lower 0.5 units box", "Illegal compute chunk/atom");
  chunk_bad("bin/1d w lower 0.5 units box", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower 0 units box", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower -1 units box", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower nan units box", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower 1e-300 units box", "too many layers");
  chunk_bad("bin/3d x lower 0.001 y lower 0.001 z lower 0.001 units box", "more than 16777216 chunks");
  chunk_bad("bin/1d x lower 0.5", "give units box");
  chunk_bad("bin/1d x lower 0.5 units lattice", "units lattice");
  chunk_bad("bin/1d x lower 0.5 units", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower 0.5 units box region r", "region");
  chunk_bad("bin/1d x lower 0.5 units box compress yes", "compress yes");
  chunk_bad("bin/1d x lower 0.5 units box ids once", "ids once");
  chunk_bad("bin/1d x lower 0.5 units box limit 5 max", "limit 5");
  chunk_bad("bin/1d x lower 0.5 units box limit", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower 0.5 units box bound x 0.1", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower 0.5 units box bound x 0.8 0.2", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower 0.5 units box discard maybe", "Illegal compute chunk/atom");
  chunk_bad("bin/1d x lower 0.5 units box what", "Illegal compute chunk/atom");
  chunk_bad("type", "style type");
  chunk_bad("molecule", "style molecule");
  chunk_bad("c_other", "style c_other");
  chunk_bad("v_var", "style v_var");
  chunk_bad("bin/1d x lower 0.5 units box 'open", "Unbalanced quotes");

  ave_ok("5 1 10 c vx vy vz fx fy fz density/number density/mass c_s[1] c_s[4] c_c c_k", 12);
  ave_ok("2 3 10 c vx norm sample ave running file out.profile overwrite title1 \"a b c\" title2 't 2' title3 x format %.10g", 1);
  ave_ok("10 1 10 c c_k norm none ave one", 1);
  ave_bad("", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c", "Illegal fix ave/chunk");
  ave_bad("0 1 10 c vx", "Illegal fix ave/chunk");
  ave_bad("5 0 10 c vx", "Illegal fix ave/chunk");
  ave_bad("5 1 0 c vx", "Illegal fix ave/chunk");
  ave_bad("3 1 10 c vx", "Illegal fix ave/chunk");
  ave_bad("5 3 10 c vx", "Illegal fix ave/chunk");
  ave_bad("5 1 x c vx", "Illegal fix ave/chunk");
  ave_bad("5 1 99999999999999999999 c vx", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c temp", "temp is not supported");
  ave_bad("5 1 10 c f_other", "f_other is not supported");
  ave_bad("5 1 10 c v_var", "v_var is not supported");
  ave_bad("5 1 10 c c_", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c c_s[", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c c_s[0]", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c c_s[1]x", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c c_[2]", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c c_s[+1]", "Illegal fix ave/chunk");   // (an index is digits and nothing else, as in LAMMPS)
  ave_bad("5 1 10 c \"c_s[ 1]\"", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c c_s]", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c c_s[1000001]", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c vx ave window 5", "ave window");
  ave_bad("5 1 10 c vx norm", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c vx norm both", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c vx bias t", "bias is not supported");
  ave_bad("5 1 10 c vx adof 3", "adof is not supported");
  ave_bad("5 1 10 c vx format %s", "format %s");
  ave_bad("5 1 10 c vx format %g%g", "format %g%g");
  ave_bad("5 1 10 c vx format %", "format %");
  ave_bad("5 1 10 c vx format %.99999g", "format");
  ave_bad("5 1 10 c vx format %lg", "format %lg");
  ave_bad("5 1 10 c vx title1", "Illegal fix ave/chunk");
  ave_bad("5 1 10 c vx what", "Illegal fix ave/chunk");
  {
    std::string many = "5 1 10 c";
    for (int k = 0; k < 25; k++) many += " vx";
    ave_bad(many, "more than 24 values");
  }
  // the layers of a coordinate, and the first valid step
  {
    sf::ChunkBins B;
    const std::string e = chunk("bin/1d x lower 0.25 units box discard yes", &B);
    const bool ok = e.empty() && sf::chunk_layer_of(B, 0, -0.1) == 3 && sf::chunk_layer_of(B, 0, 1.05) == 0 &&
                    sf::chunk_layer_of(B, 0, 0.5) == 2;
    expect(ok, "layers of -0.1, 1.05 and 0.5 in a periodic unit box", e);
    const bool sched = sf::ave_first_valid(0, 5, 1, 10) == 0 && sf::ave_first_valid(7, 5, 1, 10) == 10 &&
                       sf::ave_first_valid(0, 2, 3, 10) == 6 && sf::ave_first_valid(7, 2, 3, 10) == 16 &&
                       sf::ave_first_valid(20, 10, 1, 10) == 20;
    expect(sched, "first valid steps", "");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
