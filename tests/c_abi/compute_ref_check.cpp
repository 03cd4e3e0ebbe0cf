// compute_ref_check.cpp -- the rules of csrc/sf_compute_ref.h (what each reader of a `c_ID` / `c_ID[k]` word accepts of a
// compute of each kind) against the checks as they stood, file by file, before the registry of compute kinds existed: the
// `was_*` functions below are those checks written out over the four lookups they used, with every text copied from the
// fail(...) call named next to it (file:line of the commit before sf_compute_ref.h was added).  A stand-alone program for the
// host sanitizers (tests/test_compute_ref.py builds it with -fsanitize=address,undefined and runs it once).  Prints one line
// per case; exit status 0 when every case gave what is expected of it.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_compute_ref.h"

namespace {
int failures = 0;
int cases = 0;

void expect_same(const std::string& what, const std::string& got, const std::string& want)
{
  const bool ok = got == want;
  cases++;
  std::printf("%s %s -> %s\n", ok ? "ok  " : "FAIL", what.c_str(), got.empty() ? "(accepted)" : got.c_str());
  if (!ok) {
    std::printf("     expected: %s\n", want.empty() ? "(accepted)" : want.c_str());
    failures++;
  }
}

// what the four lookups of the old checks answered for one ID
struct Was {
  std::string name;
  int nc = 0;           // atom_compute_ncols (which answered 1 for a chunk/atom compute)
  bool chunk = false;   // chunk_compute_exists
  bool local = false;   // pair_local_exists
  int nv = 0;           // the values of compute_lookup
  int gn = 0;           // global_compute_nvalues
  bool gvec = false;    // its is_vector
  int rows = 0;         // rdf_array_rows
  int ncols = 0;        // its ncols
};

struct Case {
  Was was;
  sf::ComputeShape shape;
};

std::vector<Case> shapes()
{
  std::vector<Case> v;
  auto add = [&](const char* name, sf::ComputeKind kind, int n, bool vector, int rows, bool chunk) {
    Case c;
    c.was.name = name;
    c.shape.kind = kind;
    c.shape.n = n;
    c.shape.vector = vector;
    c.shape.rows = rows;
    c.shape.chunk = chunk;
    if (kind == sf::CK_LOCAL) c.was.local = true, c.was.nv = n;
    if (kind == sf::CK_PERATOM) c.was.nc = n, c.was.chunk = chunk;
    if (kind == sf::CK_GLOBAL) c.was.gn = n, c.was.gvec = vector;
    if (kind == sf::CK_ARRAY) c.was.rows = rows, c.was.ncols = n;
    v.push_back(c);
  };
  add("none", sf::CK_NONE, 0, false, 0, false);
  add("local1", sf::CK_LOCAL, 1, false, 0, false);
  add("local3", sf::CK_LOCAL, 3, false, 0, false);
  add("atom1", sf::CK_PERATOM, 1, false, 0, false);
  add("atom6", sf::CK_PERATOM, 6, false, 0, false);
  add("chunk", sf::CK_PERATOM, 1, false, 0, true);
  add("scalar", sf::CK_GLOBAL, 1, false, 0, false);
  add("vector3", sf::CK_GLOBAL, 3, true, 0, false);
  add("array5x3", sf::CK_ARRAY, 3, false, 5, false);
  return v;
}

std::string word_of(const std::string& id, long index) { return "c_" + id + (index > 0 ? "[" + std::to_string(index) + "]" : ""); }

// sf_dump.hip:584-597 (the c_ columns of dump custom)
std::string was_dump_custom(const Was& w, long idx, const std::string& word, const std::string& id)
{
  const int nc = w.nc;
  if (nc == 0 && w.local)   // sf_dump.hip:586
    return "Dump custom compute does not compute per-atom info: " + id + " is a compute pair/local (dump local prints its rows)";
  if (nc == 0 && w.gn > 0)   // sf_dump.hip:589
    return "Dump custom compute does not compute per-atom info: " + id + " is a global compute (fix ave/time and thermo print it)";
  if (nc == 0 && w.rows > 0)   // sf_dump.hip:592
    return "Dump custom compute does not compute per-atom info: " + id + " is a global array (fix ave/time mode vector prints it)";
  if (nc == 0) return "Could not find dump custom compute ID " + id;                                        // sf_dump.hip:594
  if (idx == 0 && nc != 1) return "Dump custom compute does not compute per-atom vector: " + word;          // sf_dump.hip:595
  if (idx > 0 && nc == 1) return "Dump custom compute does not compute per-atom array: " + word;            // sf_dump.hip:596
  if (idx > nc) return "Dump custom compute vector is accessed out-of-range: " + word;                      // sf_dump.hip:597
  return "";
}

// sf_contacts.hip:405-411 (compute_lookup) and sf_dump.hip:557-561 (the c_ columns of dump local; idx 0: no bracket)
std::string was_dump_local(const Was& w, long idx, const std::string& word, const std::string& id)
{
  if (!w.local && w.nc > 0)   // sf_contacts.hip:406
    return "Dump local compute does not compute local info: " + id + " is a per-atom compute (dump custom prints it)";
  if (!w.local && w.gn > 0)   // sf_contacts.hip:408
    return "Dump local compute does not compute local info: " + id + " is a global compute (fix ave/time and thermo print it)";
  if (!w.local && w.rows > 0)   // sf_contacts.hip:410
    return "Dump local compute does not compute local info: " + id + " is a global array (fix ave/time mode vector prints it)";
  if (!w.local) return "Could not find dump local compute ID " + id;   // sf_contacts.hip:411
  if (idx == 0) {
    if (w.nv != 1) return "Dump local compute does not compute local vector: " + word;                // sf_dump.hip:558
  } else if (idx > w.nv)
    return "Dump local compute vector is accessed out-of-range: " + word;                               // sf_dump.hip:561
  return "";
}

// sf_global.hip:390-415 (check_reduce_input)
std::string was_reduce(const Was& w, long index, const std::string& id)
{
  const int nc = w.nc;
  if (nc > 0) {
    if (index == 0 && nc != 1) return "Compute reduce compute does not calculate a per-atom vector";   // sf_global.hip:394
    if (index > 0 && nc == 1) return "Compute reduce compute does not calculate a per-atom array";     // sf_global.hip:395
    if (index > nc) return "Compute reduce compute array is accessed out-of-range";                    // sf_global.hip:396
    return "";
  }
  if (w.local) {
    const long nv = w.nv;
    if (index == 0 && nv != 1) return "Compute reduce compute does not calculate a local vector";      // sf_global.hip:403
    if (index > 0 && nv == 1) return "Compute reduce compute does not calculate a local array";        // sf_global.hip:404
    if (index > nv) return "Compute reduce compute array is accessed out-of-range";                    // sf_global.hip:405
    return "";
  }
  if (w.gn > 0)   // sf_global.hip:409
    return "Compute reduce compute calculates global values (c_" + id + " is a global compute: per-atom and local ones are reduced)";
  if (w.rows > 0)   // sf_global.hip:412
    return "Compute reduce compute calculates global values (c_" + id + " is a global array: per-atom and local ones are reduced)";
  return "Compute ID for compute reduce does not exist";   // sf_global.hip:414
}

// sf_chunk.hip:344-353 (check_compute_value)
std::string was_ave_chunk_value(const Was& w, long index)
{
  const int nc = w.nc;
  if (nc == 0 && (w.local || w.gn > 0 || w.rows > 0)) return "Fix ave/chunk compute does not calculate per-atom values";   // sf_chunk.hip:348
  if (nc == 0) return "Compute ID for fix ave/chunk does not exist";                                    // sf_chunk.hip:349
  if (index == 0 && nc != 1) return "Fix ave/chunk compute does not calculate a per-atom vector";       // sf_chunk.hip:350
  if (index > 0 && nc == 1) return "Fix ave/chunk compute does not calculate a per-atom array";         // sf_chunk.hip:351
  if (index > nc) return "Fix ave/chunk compute vector is accessed out-of-range";                       // sf_chunk.hip:352
  return "";
}

// sf_chunk.hip:608-614 (the chunk ID of a fix ave/chunk line)
std::string was_ave_chunk_id(const Was& w)
{
  if (!w.chunk) {
    if (w.nc > 0 || w.local || w.gn > 0 || w.rows > 0) return "Fix ave/chunk does not use chunk/atom compute";   // sf_chunk.hip:612
    return "Chunk/atom compute does not exist for fix ave/chunk";                                                 // sf_chunk.hip:613
  }
  return "";
}

// sf_global.hip:633-645 (check_fix_value)
std::string was_ave_time_scalar(const Was& w, long index)
{
  const bool vec = w.gvec;
  const int n = w.gn;
  if (n == 0) {
    if (w.nc > 0 || w.local || w.rows > 0)   // sf_global.hip:639
      return index == 0 ? "Fix ave/time compute does not calculate a scalar" : "Fix ave/time compute does not calculate a vector";
    return "Compute ID for fix ave/time does not exist";   // sf_global.hip:640
  }
  if (index == 0 && vec) return "Fix ave/time compute does not calculate a scalar";       // sf_global.hip:642
  if (index > 0 && !vec) return "Fix ave/time compute does not calculate a vector";       // sf_global.hip:643
  if (index > n) return "Fix ave/time compute vector is accessed out-of-range";           // sf_global.hip:644
  return "";
}

// sf_global.hip:649-661 (check_fix_column)
std::string was_ave_time_vector(const Was& w, long index, int nrows)
{
  const int ncols = w.ncols, rows = w.rows;
  if (rows == 0) {
    if (w.gn > 0 || w.nc > 0 || w.local) return "Fix ave/time compute does not calculate an array";   // sf_global.hip:655
    return "Compute ID for fix ave/time does not exist";                                               // sf_global.hip:656
  }
  if (index > ncols) return "Fix ave/time compute array is accessed out-of-range";                     // sf_global.hip:658
  if (nrows > 0 && rows != nrows) return "Fix ave/time columns must all be the same length";           // sf_global.hip:659
  return "";
}

// sf_histo.hip:209-214 (check_values: what kind a value is)
std::string was_ave_histo_kind(const Was& w, const std::string& id)
{
  if (w.nc > 0 || w.local || w.gn > 0) return "";
  if (w.rows > 0)   // sf_histo.hip:213
    return "Fix ave/histo compute does not calculate a global scalar or vector (c_" + id + " is a global array, which is not binned)";
  return "Compute ID for fix ave/histo does not exist";   // sf_histo.hip:214
}

// sf_histo.hip:224-250 (check_values: the index against the kind the values agree on)
std::string was_ave_histo_index(const Was& w, long index, bool scalar_mode)
{
  if (w.nc > 0) {
    const int nc = w.nc;
    if (index == 0 && nc != 1) return "Fix ave/histo compute does not calculate a per-atom vector";   // sf_histo.hip:228
    if (index > 0 && nc == 1) return "Fix ave/histo compute does not calculate a per-atom array";     // sf_histo.hip:229
    if (index > nc) return "Fix ave/histo compute array is accessed out-of-range";                    // sf_histo.hip:230
  } else if (w.local) {
    const long nv = w.nv;
    if (index == 0 && nv != 1) return "Fix ave/histo compute does not calculate a local vector";      // sf_histo.hip:235
    if (index > 0 && nv == 1) return "Fix ave/histo compute does not calculate a local array";        // sf_histo.hip:236
    if (index > nv) return "Fix ave/histo compute array is accessed out-of-range";                    // sf_histo.hip:237
  } else {
    const bool vec = w.gvec;
    const int n = w.gn;
    if (scalar_mode) {
      if (index == 0 && vec) return "Fix ave/histo compute does not calculate a global scalar";       // sf_histo.hip:242
      if (index > 0 && !vec) return "Fix ave/histo compute does not calculate a global vector";       // sf_histo.hip:243
      if (index > n) return "Fix ave/histo compute vector is accessed out-of-range";                  // sf_histo.hip:244
    } else {
      if (index > 0) return "Fix ave/histo compute does not calculate a global array";                // sf_histo.hip:246
      if (!vec) return "Fix ave/histo compute does not calculate a global vector";                    // sf_histo.hip:247
    }
  }
  return "";
}

// sf_thermo.hip:371-382 (check_compute_cols)
std::string was_thermo(const Was& w, long index, const std::string& id)
{
  const bool vec = w.gvec;
  const int n = w.gn;
  if (n == 0) {
    if (w.nc > 0 || w.local || w.rows > 0)   // sf_thermo.hip:376
      return index == 0 ? "Thermo compute does not compute scalar" : "Thermo compute does not compute vector";
    return "Could not find thermo custom compute ID: " + id;   // sf_thermo.hip:377
  }
  if (index == 0 && vec) return "Thermo compute does not compute scalar";         // sf_thermo.hip:379
  if (index > 0 && !vec) return "Thermo compute does not compute vector";         // sf_thermo.hip:380
  if (index > n) return "Thermo compute vector is accessed out-of-range";         // sf_thermo.hip:381
  return "";
}

// sf_compute_atom.hip:471-482 (atom_compute_values, behind sf_lammps_compute_atom)
std::string was_get_atom(const Was& w, const std::string& id)
{
  if (w.nc > 0) return "";
  if (w.gn > 0) return "compute " + id + " does not calculate per-atom values (it is a global compute)";   // sf_compute_atom.hip:479
  if (w.rows > 0)   // sf_compute_atom.hip:481
    return "compute " + id + " does not calculate per-atom values (it is a global array: sf_lammps_compute_array returns it)";
  return "Could not find compute ID " + id;   // sf_compute_atom.hip:482
}

// sf_global.hip:958-968 (sf_lammps_compute_global)
std::string was_get_global(const Was& w, const std::string& id)
{
  if (w.gn == 0) {
    if (w.nc > 0 || w.local)   // sf_global.hip:962
      return "compute " + id + " does not calculate a global scalar or vector (sf_lammps_compute_atom and sf_lammps_get_contacts "
             "return per-atom and local values)";
    if (w.rows > 0)   // sf_global.hip:965
      return "compute " + id + " does not calculate a global scalar or vector (it is a global array: sf_lammps_compute_array returns "
             "it)";
    return "Could not find compute ID " + id;   // sf_global.hip:967
  }
  return "";
}

// sf_nbr.hip:615-621 (sf_lammps_compute_array)
std::string was_get_array(const Was& w, const std::string& id)
{
  if (w.rows == 0) {
    if (w.nc > 0 || w.local || w.gn > 0) return "compute " + id + " does not calculate a global array (compute rdf does)";   // sf_nbr.hip:619
    return "Could not find compute ID " + id;                                                                               // sf_nbr.hip:620
  }
  return "";
}

// sf_compute_atom.hip:532-537 (atom_compute_cost)
std::string was_atom_cost(const Was& w, const std::string& id)
{
  if (w.chunk) return "compute " + id + " is a chunk/atom compute: sf_lammps_ave_chunk_cost times its pass";   // sf_compute_atom.hip:536
  if (w.nc == 0) return "Could not find compute ID " + id;                                                      // sf_compute_atom.hip:537
  return "";
}

}  // namespace

int main()
{
  for (const Case& c : shapes()) {
    const Was& w = c.was;
    const sf::ComputeShape& s = c.shape;
    const std::string& id = w.name;
    const long indices[4] = {0, 1, s.n, s.n + 1};
    for (long k : indices) {
      const std::string word = word_of(id, k), at = " " + word;
      expect_same("dump custom" + at, sf::check_dump_custom(s, k, word, id), was_dump_custom(w, k, word, id));
      expect_same("dump local" + at, sf::check_dump_local(s, k, word, id), was_dump_local(w, k, word, id));
      expect_same("compute reduce" + at, sf::check_reduce_input(s, k, id), was_reduce(w, k, id));
      expect_same("ave/chunk value" + at, sf::check_ave_chunk_value(s, k), was_ave_chunk_value(w, k));
      expect_same("ave/time scalar" + at, sf::check_ave_time_scalar(s, k), was_ave_time_scalar(w, k));
      for (int nrows : {0, 5, 4})
        expect_same("ave/time vector" + at + " rows " + std::to_string(nrows), sf::check_ave_time_vector(s, k, nrows),
                    was_ave_time_vector(w, k, nrows));
      if (was_ave_histo_kind(w, id).empty())
        for (bool scalar_mode : {true, false})
          expect_same(std::string("ave/histo ") + (scalar_mode ? "scalar" : "vector") + at,
                      sf::check_ave_histo_index(s, k, scalar_mode), was_ave_histo_index(w, k, scalar_mode));
      expect_same("thermo" + at, sf::check_thermo(s, k, id), was_thermo(w, k, id));
    }
    expect_same("ave/chunk chunk ID " + id, sf::check_ave_chunk_id(s), was_ave_chunk_id(w));
    expect_same("ave/histo kind " + id, sf::check_ave_histo_kind(s, id), was_ave_histo_kind(w, id));
    expect_same("compute_atom " + id, sf::check_get_atom(s, id), was_get_atom(w, id));
    expect_same("compute_global " + id, sf::check_get_global(s, id), was_get_global(w, id));
    expect_same("compute_array " + id, sf::check_get_array(s, id), was_get_array(w, id));
    expect_same("compute_atom_cost " + id, sf::check_atom_cost(s, id), was_atom_cost(w, id));
  }
  // a few texts spelled out whole, so that a slip shared by both sides above would still show
  sf::ComputeShape none, scalar;
  scalar.kind = sf::CK_GLOBAL;
  scalar.n = 1;
  expect_same("spelled: dump custom of a global", sf::check_dump_custom(scalar, 0, "c_t", "t"),
              "Dump custom compute does not compute per-atom info: t is a global compute (fix ave/time and thermo print it)");
  expect_same("spelled: thermo of nothing", sf::check_thermo(none, 0, "t"), "Could not find thermo custom compute ID: t");
  expect_same("spelled: ave/time c_t[2] of a scalar", sf::check_ave_time_scalar(scalar, 2), "Fix ave/time compute does not calculate a vector");
  expect_same("spelled: thermo of a scalar", sf::check_thermo(scalar, 0, "t"), "");
  std::printf("%d cases, %d failures\n", cases, failures);
  return failures == 0 ? 0 : 1;
}
