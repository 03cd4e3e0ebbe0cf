// sf_chunk.h -- `compute ID group chunk/atom bin/1d|2d|3d ...` and `fix ID group ave/chunk Nevery Nrepeat Nfreq chunkID
// value ...` (sf_chunk.hip): atoms assigned to spatial bins and per-bin sums reduced on the GPU, averaged over time and
// written as profiles.  The compute is a per-atom compute (one column, the chunk ID): compute_command (sf_compute_ids.hip) hands it
// over through sf_compute_atom.hip, whose kind forwards here, so `c_ID` in dump custom and sf_lammps_compute_atom see it unchanged.
// `compute ID group chunk/atom c_CID ...`, a chunk ID read from a per-atom compute, is held by sf_pchunk.hip: the functions of
// the compute below forward to it what they do not hold.
#pragma once
#include <string>
#include <vector>

namespace sf {
struct SfLammps;
struct ComputeShape;

// ---- the compute (called by sf_compute_atom.hip for the style chunk/atom and for IDs it does not hold) ----
void chunk_compute_define(SfLammps& L, const std::vector<std::string>& w);
// one column, chunk set; false: no compute chunk/atom has this ID
bool chunk_compute_shape(const SfLammps& L, const std::string& id, ComputeShape* s);
void chunk_compute_remove(SfLammps& L, const std::string& id);
// the chunk IDs as doubles, one per owned atom (0: outside the group, or discarded), assigned once per step
const double* chunk_compute_values(SfLammps& L, const std::string& id);
// the state changed at an unchanged step: assign and group again when asked next (computes_invalidate of sf_compute_ids.hip)
void chunk_invalidate(SfLammps& L);

// ---- the fix (its ID space, unfix and the run's cuts: sf_ave_fix.h) ----
// `fix ID group ave/chunk ...` from the whole line (its title keywords may be quoted)
void ave_chunk_fix_command(SfLammps& L, const std::string& line);

// ---- the run (ave_fix_step_due of sf_ave_fix.hip) ----
// the samples (and outputs) due at the engine's current step that were not taken yet
void ave_chunk_sample_due(SfLammps& L);
}  // namespace sf
