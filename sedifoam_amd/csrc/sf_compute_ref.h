// sf_compute_ref.h -- what every reader of a `c_ID` / `c_ID[k]` word accepts, given the shape of the compute behind the ID
// (compute_shape of sf_compute_ids.h).  Host-only, nothing but the standard library, so that the rules and their texts can be
// compiled into a stand-alone program and run without a GPU (tests/c_abi/compute_ref_check.cpp).  One function per reader:
// it returns an empty string, or the error text ([3P] LAMMPS wording where LAMMPS has the rule).  `index` is k of c_ID[k],
// 0 where none was typed.
#pragma once
#include <string>

namespace sf {

enum ComputeKind { CK_NONE, CK_LOCAL, CK_PERATOM, CK_GLOBAL, CK_ARRAY };

struct ComputeShape {
  ComputeKind kind = CK_NONE;
  int n = 0;             // values of a local row, columns of a per-atom compute, length of a global compute, columns of an array
  bool vector = false;   // a global compute: read as c_ID[k]
  int rows = 0;          // an array
  bool chunk = false;    // a per-atom compute: a chunk/atom one (sf_chunk.hip, sf_pchunk.hip)
  bool rows_vary = false;   // an array: `rows` is that of the last evaluation and may change with the next (a per-chunk compute
                            // whose chunk/atom compute has compress yes or nchunk every; sf_pchunk.hip)
};

// ---- dump custom: c_ID names a per-atom vector, c_ID[k] a column of a per-atom array ([3P] DumpCustom::parse_fields) ----
inline std::string check_dump_custom(const ComputeShape& s, long index, const std::string& word, const std::string& id)
{
  const std::string no = "Dump custom compute does not compute per-atom info: " + id;
  if (s.kind == CK_LOCAL) return no + " is a compute pair/local (dump local prints its rows)";
  if (s.kind == CK_GLOBAL) return no + " is a global compute (fix ave/time and thermo print it)";
  if (s.kind == CK_ARRAY) return no + " is a global array (fix ave/time mode vector prints it)";
  if (s.kind == CK_NONE) return "Could not find dump custom compute ID " + id;
  if (index == 0 && s.n != 1) return "Dump custom compute does not compute per-atom vector: " + word;
  if (index > 0 && s.n == 1) return "Dump custom compute does not compute per-atom array: " + word;
  if (index > s.n) return "Dump custom compute vector is accessed out-of-range: " + word;
  return std::string();
}

// ---- dump local: the values of one compute pair/local ([3P] DumpLocal::parse_fields) ----
inline std::string check_dump_local(const ComputeShape& s, long index, const std::string& word, const std::string& id)
{
  const std::string no = "Dump local compute does not compute local info: " + id;
  if (s.kind == CK_PERATOM) return no + " is a per-atom compute (dump custom prints it)";
  if (s.kind == CK_GLOBAL) return no + " is a global compute (fix ave/time and thermo print it)";
  if (s.kind == CK_ARRAY) return no + " is a global array (fix ave/time mode vector prints it)";
  if (s.kind == CK_NONE) return "Could not find dump local compute ID " + id;
  if (index == 0 && s.n != 1) return "Dump local compute does not compute local vector: " + word;
  if (index > s.n) return "Dump local compute vector is accessed out-of-range: " + word;
  return std::string();
}

// ---- a c_ input of compute reduce: per-atom and local values are reduced ----
inline std::string check_reduce_input(const ComputeShape& s, long index, const std::string& id)
{
  if (s.kind == CK_PERATOM) {
    if (index == 0 && s.n != 1) return "Compute reduce compute does not calculate a per-atom vector";
    if (index > 0 && s.n == 1) return "Compute reduce compute does not calculate a per-atom array";
    if (index > s.n) return "Compute reduce compute array is accessed out-of-range";
    return std::string();
  }
  if (s.kind == CK_LOCAL) {
    if (index == 0 && s.n != 1) return "Compute reduce compute does not calculate a local vector";
    if (index > 0 && s.n == 1) return "Compute reduce compute does not calculate a local array";
    if (index > s.n) return "Compute reduce compute array is accessed out-of-range";
    return std::string();
  }
  const std::string global = "Compute reduce compute calculates global values (c_" + id;
  if (s.kind == CK_GLOBAL) return global + " is a global compute: per-atom and local ones are reduced)";
  if (s.kind == CK_ARRAY) return global + " is a global array: per-atom and local ones are reduced)";
  return "Compute ID for compute reduce does not exist";
}

// ---- fix ave/chunk: the column of a c_ value, and the chunk ID ----
inline std::string check_ave_chunk_value(const ComputeShape& s, long index)
{
  if (s.kind == CK_NONE) return "Compute ID for fix ave/chunk does not exist";
  if (s.kind != CK_PERATOM) return "Fix ave/chunk compute does not calculate per-atom values";
  if (index == 0 && s.n != 1) return "Fix ave/chunk compute does not calculate a per-atom vector";
  if (index > 0 && s.n == 1) return "Fix ave/chunk compute does not calculate a per-atom array";
  if (index > s.n) return "Fix ave/chunk compute vector is accessed out-of-range";
  return std::string();
}

inline std::string check_ave_chunk_id(const ComputeShape& s)
{
  if (s.kind == CK_NONE) return "Chunk/atom compute does not exist for fix ave/chunk";
  if (!s.chunk) return "Fix ave/chunk does not use chunk/atom compute";
  return std::string();
}

// ---- fix ave/time: a global scalar or c_ID[k] of a global vector; mode vector: column k of a global array ----
inline std::string check_ave_time_scalar(const ComputeShape& s, long index)
{
  if (s.kind == CK_NONE) return "Compute ID for fix ave/time does not exist";
  if (s.kind != CK_GLOBAL)
    return index == 0 ? "Fix ave/time compute does not calculate a scalar" : "Fix ave/time compute does not calculate a vector";
  if (index == 0 && s.vector) return "Fix ave/time compute does not calculate a scalar";
  if (index > 0 && !s.vector) return "Fix ave/time compute does not calculate a vector";
  if (index > s.n) return "Fix ave/time compute vector is accessed out-of-range";
  return std::string();
}

// nrows: the rows of the fix's earlier columns, 0 where this is the first
inline std::string check_ave_time_vector(const ComputeShape& s, long index, int nrows)
{
  if (s.kind == CK_NONE) return "Compute ID for fix ave/time does not exist";
  if (s.kind != CK_ARRAY) return "Fix ave/time compute does not calculate an array";
  if (index > s.n) return "Fix ave/time compute array is accessed out-of-range";
  if (s.rows_vary)
    return "Fix ave/time compute array has a varying number of rows (mode vector takes a per-chunk compute only when its "
           "chunk/atom compute is compress no nchunk once)";
  if (nrows > 0 && s.rows != nrows) return "Fix ave/time columns must all be the same length";
  return std::string();
}

// ---- fix ave/histo: first what kind a value is (a global array is not binned), then, once the values of the fix agree on
// a kind, the index against it.  scalar_mode: `mode scalar` ----
inline std::string check_ave_histo_kind(const ComputeShape& s, const std::string& id)
{
  if (s.kind == CK_ARRAY)
    return "Fix ave/histo compute does not calculate a global scalar or vector (c_" + id + " is a global array, which is not binned)";
  if (s.kind == CK_NONE) return "Compute ID for fix ave/histo does not exist";
  return std::string();
}

inline std::string check_ave_histo_index(const ComputeShape& s, long index, bool scalar_mode)
{
  if (s.kind == CK_PERATOM) {
    if (index == 0 && s.n != 1) return "Fix ave/histo compute does not calculate a per-atom vector";
    if (index > 0 && s.n == 1) return "Fix ave/histo compute does not calculate a per-atom array";
    if (index > s.n) return "Fix ave/histo compute array is accessed out-of-range";
  } else if (s.kind == CK_LOCAL) {
    if (index == 0 && s.n != 1) return "Fix ave/histo compute does not calculate a local vector";
    if (index > 0 && s.n == 1) return "Fix ave/histo compute does not calculate a local array";
    if (index > s.n) return "Fix ave/histo compute array is accessed out-of-range";
  } else if (scalar_mode) {
    if (index == 0 && s.vector) return "Fix ave/histo compute does not calculate a global scalar";
    if (index > 0 && !s.vector) return "Fix ave/histo compute does not calculate a global vector";
    if (index > s.n) return "Fix ave/histo compute vector is accessed out-of-range";
  } else {
    if (index > 0) return "Fix ave/histo compute does not calculate a global array";   // (no compute here has one)
    if (!s.vector) return "Fix ave/histo compute does not calculate a global vector";
  }
  return std::string();
}

// ---- a c_ column of thermo_style custom ([3P] Thermo::parse_fields) ----
inline std::string check_thermo(const ComputeShape& s, long index, const std::string& id)
{
  if (s.kind == CK_NONE) return "Could not find thermo custom compute ID: " + id;
  if (s.kind != CK_GLOBAL) return index == 0 ? "Thermo compute does not compute scalar" : "Thermo compute does not compute vector";
  if (index == 0 && s.vector) return "Thermo compute does not compute scalar";
  if (index > 0 && !s.vector) return "Thermo compute does not compute vector";
  if (index > s.n) return "Thermo compute vector is accessed out-of-range";
  return std::string();
}

// ---- the getters sf_lammps_compute_atom / _global / _array, and sf_lammps_compute_atom_cost ----
inline std::string check_get_atom(const ComputeShape& s, const std::string& id)
{
  if (s.kind == CK_GLOBAL) return "compute " + id + " does not calculate per-atom values (it is a global compute)";
  if (s.kind == CK_ARRAY)
    return "compute " + id + " does not calculate per-atom values (it is a global array: sf_lammps_compute_array returns it)";
  if (s.kind != CK_PERATOM) return "Could not find compute ID " + id;
  return std::string();
}

inline std::string check_get_global(const ComputeShape& s, const std::string& id)
{
  if (s.kind == CK_PERATOM || s.kind == CK_LOCAL)
    return "compute " + id + " does not calculate a global scalar or vector (sf_lammps_compute_atom and sf_lammps_get_contacts "
           "return per-atom and local values)";
  if (s.kind == CK_ARRAY)
    return "compute " + id + " does not calculate a global scalar or vector (it is a global array: sf_lammps_compute_array returns "
           "it)";
  if (s.kind == CK_NONE) return "Could not find compute ID " + id;
  return std::string();
}

inline std::string check_get_array(const ComputeShape& s, const std::string& id)
{
  if (s.kind == CK_NONE) return "Could not find compute ID " + id;
  if (s.kind != CK_ARRAY) return "compute " + id + " does not calculate a global array (compute rdf does)";
  return std::string();
}

inline std::string check_atom_cost(const ComputeShape& s, const std::string& id)
{
  if (s.chunk) return "compute " + id + " is a chunk/atom compute: sf_lammps_ave_chunk_cost times its pass";
  if (s.kind != CK_PERATOM) return "Could not find compute ID " + id;
  return std::string();
}

}  // namespace sf
