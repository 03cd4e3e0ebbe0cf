// sf_pchunk.h -- chunks that a compute defines, and what is reduced over them (sf_pchunk.hip):
// `compute ID group chunk/atom c_CID | c_CID[k] [compress yes|no] [nchunk once|every] ...`, a chunk/atom compute whose chunk ID
// is a column of a per-atom compute (sf_chunk.hip forwards to it what it does not hold, as sf_compute_atom.hip forwards to
// sf_chunk.hip), and the per-chunk computes `property/chunk`, `com/chunk`, `vcm/chunk` and `gyration/chunk`, global arrays of
// Nchunk rows that plug into the registry of sf_compute_ids.h as pchunk_compute_kind().
#pragma once
#include <string>
#include <vector>

#include "sf_handles.h"

namespace sf {
struct ComputeShape;

// ---- the chunk/atom compute over c_CID (called by sf_chunk.hip) ----
void pchunk_atom_define(SfLammps& L, const std::vector<std::string>& w);
// one column, chunk set; false: no such compute has this ID
bool pchunk_atom_shape(const SfLammps& L, const std::string& id, ComputeShape* s);
void pchunk_atom_remove(SfLammps& L, const std::string& id);
// the chunk IDs as doubles, one per owned atom, assigned once per step; nullptr: no such compute has this ID
const double* pchunk_atom_values(SfLammps& L, const std::string& id);

// ---- the per-chunk computes ----
// is `id` a per-chunk compute?
bool pchunk_holds(const SfLammps& L, const std::string& id);
// its chunk/atom compute is evaluated when it is `nchunk once` and has not fixed its rows yet, so that compute_shape knows them
// (fix ave/time mode vector calls this before it asks for the shape); nothing where `id` is not a per-chunk compute
void pchunk_prepare(SfLammps& L, const std::string& id);
// the array of per-chunk compute `id` on the device, row-major [rows][ncols], on the state as it stands (evaluated first when
// it is stale; no copy besides the 4 bytes of Nchunk)
const double* pchunk_array_device(SfLammps& L, const std::string& id, int* rows, int* ncols);
// "compute property/chunk" (...) when a per-chunk compute names chunk/atom compute `id`, "compute chunk/atom" when a chunk/atom
// compute reads per-atom compute `id`; nullptr: none does (uncompute asks)
const char* pchunk_uses_compute(const SfLammps& L, const std::string& id);

}  // namespace sf
