// pchunk_parse_check.cpp -- parse_chunk_atom_compute, parse_pchunk and the checks beside them of csrc/sf_pchunk_parse.h
// (host-only) over well- and ill-formed lines, and the old parser's refusals that stay, as a stand-alone program for the host
// sanitizers (tests/test_pchunk_parse.py builds it with -fsanitize=address,undefined and runs it once).  Prints one line per
// case; exit status 0 when every case gave what is expected of it.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_chunk_parse.h"
#include "../../sedifoam_amd/csrc/sf_pchunk_parse.h"

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

void atom_ok(const std::string& args, const std::string& cid, long index, bool compress, bool every)
{
  sf::ChunkRefSpec S;
  const std::vector<std::string> w = words("compute cc all chunk/atom " + args);
  const std::string e = sf::parse_chunk_atom_compute(w, &S);
  expect(sf::chunk_style_is_compute(w) && e.empty() && S.cid == cid && S.index == index && S.compress == compress &&
             S.nchunk_every == every && S.rows_fixed() == (!compress && !every),
         "chunk/atom " + args, e);
}

// refused with a text that holds `part`; what is refused leaves the caller's spec alone
void atom_bad(const std::string& args, const std::string& part)
{
  sf::ChunkRefSpec S;
  S.cid = "untouched";
  const std::string e = sf::parse_chunk_atom_compute(words("compute cc all chunk/atom " + args), &S);
  expect(!e.empty() && e.find(part) != std::string::npos && S.cid == "untouched" && S.index == 0 && !S.compress, "chunk/atom " + args, e);
}

void pchunk_ok(const std::string& line, int style, int ncols, bool id, bool tensor)
{
  sf::PChunkSpec S;
  const std::string e = sf::parse_pchunk(words(line), &S);
  expect(e.empty() && S.style == style && S.chunk == "cc" && S.ncols() == ncols && S.wants_id() == id && S.tensor == tensor, line, e);
}

void pchunk_bad(const std::string& line, const std::string& part)
{
  sf::PChunkSpec S;
  S.chunk = "untouched";
  const std::string e = sf::parse_pchunk(words(line), &S);
  expect(!e.empty() && e.find(part) != std::string::npos && S.chunk == "untouched" && S.props.empty() && !S.tensor, line, e);
}

sf::ComputeShape shape(sf::ComputeKind kind, int n, bool chunk = false)
{
  sf::ComputeShape s;
  s.kind = kind;
  s.n = n;
  s.chunk = chunk;
  return s;
}
}  // namespace

int main()
{
  const std::string illegal = "Illegal compute chunk/atom command";
  // ---- compute chunk/atom c_CID ----
  atom_ok("c_cl", "cl", 0, false, false);   // (compress no nchunk once: the defaults)
  atom_ok("c_cl[2]", "cl", 2, false, false);
  atom_ok("c_cl compress yes", "cl", 0, true, true);
  atom_ok("c_cl compress yes nchunk every", "cl", 0, true, true);
  atom_ok("c_cl nchunk every compress yes", "cl", 0, true, true);
  atom_ok("c_cl compress no", "cl", 0, false, false);
  atom_ok("c_cl nchunk once", "cl", 0, false, false);
  atom_ok("c_cl nchunk every", "cl", 0, false, true);
  atom_ok("c_p[1] nchunk every ids every limit 0 discard yes pbc no compress no", "p", 1, false, true);
  atom_ok("c_cl compress yes compress no", "cl", 0, false, false);   // (the last one holds, as in LAMMPS' keyword loops)
  atom_bad("c_cl compress yes nchunk once", "nchunk once is not supported with compress yes");
  atom_bad("c_cl nchunk once compress yes", "nchunk once is not supported with compress yes");
  atom_bad("c_cl discard no", "discard no is not supported");
  atom_bad("c_cl discard mixed", "discard mixed is not supported");
  atom_bad("c_cl ids once", "ids once is not supported");
  atom_bad("c_cl ids nfreq", "ids nfreq is not supported");
  atom_bad("c_cl limit 4", "limit 4 is not supported");
  atom_bad("c_cl limit 4 max", "limit 4 is not supported");
  atom_bad("c_cl region r", "region is not supported");
  atom_bad("c_cl bound x 0 1", "bound is not supported");
  atom_bad("c_cl units box", "units is not supported");
  atom_bad("c_cl pbc yes", "pbc yes is not supported");
  for (const char* s : {"c_", "c_cl[0]", "c_cl[", "c_cl[1", "c_cl[-1]", "c_cl[1]x", "c_cl[a]", "c_cl[1][2]", "c_cl compress", "c_cl compress maybe",
                        "c_cl nchunk", "c_cl nchunk never", "c_cl ids", "c_cl ids sometimes", "c_cl limit", "c_cl limit -1", "c_cl limit x",
                        "c_cl discard", "c_cl discard perhaps", "c_cl pbc", "c_cl pbc maybe", "c_cl extra", "c_cl extra yes", "c_cl Compress yes",
                        "c_cl '' yes", "c_cl compress ''"})
    atom_bad(s, illegal);
  {
    sf::ChunkRefSpec S;
    const std::vector<std::string> w = words("compute cc all chunk/atom");
    expect(!sf::chunk_style_is_compute(w) && sf::parse_chunk_atom_compute(w, &S) == illegal, "chunk/atom (four words)", "");
    for (const char* s : {"bin/1d", "molecule", "type", "v_x", "f_x", "C_cl", ""})
      expect(!sf::chunk_style_is_compute(words(std::string("compute cc all chunk/atom ") + s + " x")), std::string("style '") + s + "'", "");
  }

  // ---- the old parser goes on refusing what it refused ----
  {
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    const int per[3] = {1, 0, 1};
    sf::ChunkBins B;
    std::string e = sf::parse_chunk_atom(words("compute c all chunk/atom molecule"), lo, hi, per, &B);
    expect(e == "compute chunk/atom: style molecule is not supported (bin/1d, bin/2d and bin/3d are)", "chunk/atom molecule", e);
    e = sf::parse_chunk_atom(words("compute c all chunk/atom c_other"), lo, hi, per, &B);
    expect(e == "compute chunk/atom: style c_other is not supported (bin/1d, bin/2d and bin/3d are)", "chunk/atom c_other (old parser)", e);
    e = sf::parse_chunk_atom(words("compute c all chunk/atom bin/1d y lower 0.1 units box compress yes"), lo, hi, per, &B);
    expect(e == "compute chunk/atom: compress yes is not supported (compress no is)", "bin/1d compress yes", e);
  }

  // ---- the column behind c_CID ----
  using sf::check_chunk_atom_value;
  expect(check_chunk_atom_value(shape(sf::CK_PERATOM, 1), 0).empty(), "c_ID of one column", "");
  expect(check_chunk_atom_value(shape(sf::CK_PERATOM, 2), 2).empty(), "c_ID[2] of two columns", "");
  expect(check_chunk_atom_value(shape(sf::CK_PERATOM, 1, true), 0).empty(), "c_ID of a chunk/atom compute", "");
  expect(check_chunk_atom_value(shape(sf::CK_NONE, 0), 0) == "Compute ID for compute chunk/atom does not exist", "no compute", "");
  expect(check_chunk_atom_value(shape(sf::CK_GLOBAL, 3), 1) == "Compute chunk/atom compute does not calculate per-atom values", "global", "");
  expect(check_chunk_atom_value(shape(sf::CK_ARRAY, 3), 1) == "Compute chunk/atom compute does not calculate per-atom values", "array", "");
  expect(check_chunk_atom_value(shape(sf::CK_LOCAL, 3), 1) == "Compute chunk/atom compute does not calculate per-atom values", "local", "");
  expect(check_chunk_atom_value(shape(sf::CK_PERATOM, 2), 0) == "Compute chunk/atom compute does not calculate a per-atom vector", "c_ID of two", "");
  expect(check_chunk_atom_value(shape(sf::CK_PERATOM, 1), 1) == "Compute chunk/atom compute does not calculate a per-atom array", "c_ID[1] of one", "");
  expect(check_chunk_atom_value(shape(sf::CK_PERATOM, 2), 3) == "Compute chunk/atom compute vector is accessed out-of-range", "c_ID[3] of two", "");

  // ---- the per-chunk computes ----
  pchunk_ok("compute n all property/chunk cc count", sf::PC_PROPERTY, 1, false, false);
  pchunk_ok("compute n all property/chunk cc count id", sf::PC_PROPERTY, 2, true, false);
  pchunk_ok("compute n all property/chunk cc id count", sf::PC_PROPERTY, 2, true, false);
  pchunk_ok("compute n all property/chunk cc id", sf::PC_PROPERTY, 1, true, false);
  pchunk_ok("compute x all com/chunk cc", sf::PC_COM, 3, false, false);
  pchunk_ok("compute v all vcm/chunk cc", sf::PC_VCM, 3, false, false);
  pchunk_ok("compute g all gyration/chunk cc", sf::PC_GYRATION, 1, false, false);
  pchunk_ok("compute g all gyration/chunk cc tensor", sf::PC_GYRATION, 6, false, true);
  pchunk_bad("compute n all property/chunk", "Illegal compute property/chunk command");
  pchunk_bad("compute n all property/chunk cc", "Illegal compute property/chunk command");
  pchunk_bad("compute n all property/chunk cc mass", "Illegal compute property/chunk command");
  pchunk_bad("compute n all property/chunk cc count Count", "Illegal compute property/chunk command");
  pchunk_bad("compute n all property/chunk '' count", "Illegal compute property/chunk command");
  pchunk_bad("compute n all property/chunk cc coord1", "coord1 is not supported");
  pchunk_bad("compute n all property/chunk cc count coord2", "coord2 is not supported");
  pchunk_bad("compute n all property/chunk cc coord3 id", "coord3 is not supported");
  pchunk_bad("compute n all property/chunk c_cc count", "give the ID of the chunk/atom compute itself (cc, not c_cc)");
  pchunk_bad("compute x all com/chunk", "Illegal compute com/chunk command");
  pchunk_bad("compute x all com/chunk cc extra", "Illegal compute com/chunk command");
  pchunk_bad("compute x all com/chunk c_cc", "give the ID of the chunk/atom compute itself (cc, not c_cc)");
  pchunk_bad("compute v all vcm/chunk", "Illegal compute vcm/chunk command");
  pchunk_bad("compute v all vcm/chunk cc tensor", "Illegal compute vcm/chunk command");
  pchunk_bad("compute g all gyration/chunk", "Illegal compute gyration/chunk command");
  pchunk_bad("compute g all gyration/chunk cc Tensor", "Illegal compute gyration/chunk command");
  pchunk_bad("compute g all gyration/chunk cc tensor yes", "Illegal compute gyration/chunk command");
  pchunk_bad("compute g all inertia/chunk cc", "Illegal compute command");
  pchunk_bad("compute g all", "Illegal compute command");
  for (const char* s : {"property/chunk", "com/chunk", "vcm/chunk", "gyration/chunk"})
    expect(sf::pchunk_style_of(s) >= 0 && std::string(sf::pchunk_style_name(sf::pchunk_style_of(s))) == s, s, "");
  for (const char* s : {"inertia/chunk", "msd/chunk", "chunk/atom", "com", ""})
    expect(sf::pchunk_style_of(s) < 0, std::string("style '") + s + "'", "");

  // ---- what CHUNKID must be ----
  {
    sf::PChunkSpec count, id;
    sf::parse_pchunk(words("compute n all property/chunk cc count"), &count);
    sf::parse_pchunk(words("compute n all property/chunk cc count id"), &id);
    const sf::ComputeShape chunk = shape(sf::CK_PERATOM, 1, true);
    expect(sf::check_pchunk_chunk(count, chunk, true, false).empty(), "count over compress no", "");
    expect(sf::check_pchunk_chunk(id, chunk, true, true).empty(), "id over compress yes", "");
    std::string e = sf::check_pchunk_chunk(id, chunk, true, false);
    expect(e.find("id is not supported without compress yes") != std::string::npos, "id over compress no", e);
    e = sf::check_pchunk_chunk(count, shape(sf::CK_NONE, 0), false, false);
    expect(e == "Chunk/atom compute does not exist for compute property/chunk", "no chunk compute", e);
    e = sf::check_pchunk_chunk(count, shape(sf::CK_PERATOM, 1), false, false);
    expect(e == "Compute property/chunk does not use chunk/atom compute", "a per-atom compute that is no chunk compute", e);
    e = sf::check_pchunk_chunk(count, chunk, false, false);
    expect(e.find("is a bin style") != std::string::npos, "a bin-style chunk compute", e);
  }

  // ---- fix ave/time mode vector and the rows of an array ----
  {
    sf::ComputeShape a = shape(sf::CK_ARRAY, 3);
    a.rows = 7;
    expect(sf::check_ave_time_vector(a, 2, 0).empty() && sf::check_ave_time_vector(a, 2, 7).empty(), "fixed rows", "");
    expect(sf::check_ave_time_vector(a, 2, 8) == "Fix ave/time columns must all be the same length", "other rows", "");
    a.rows_vary = true;
    const std::string e = sf::check_ave_time_vector(a, 2, 0);
    expect(e.find("varying number of rows") != std::string::npos, "varying rows", e);
    expect(!sf::ComputeShape().rows_vary, "rows_vary is false by default", "");
  }

  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
