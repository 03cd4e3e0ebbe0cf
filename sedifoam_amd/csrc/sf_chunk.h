// sf_chunk.h -- `compute ID group chunk/atom bin/1d|2d|3d ...` and `fix ID group ave/chunk Nevery Nrepeat Nfreq chunkID
// value ...` (sf_chunk.hip): atoms assigned to spatial bins and per-bin sums reduced on the GPU, averaged over time and
// written as profiles.  The compute is a per-atom compute (one column, the chunk ID): compute_command hands it over through
// sf_compute_atom.hip, whose queries forward here, so `c_ID` in dump custom and sf_lammps_compute_atom see it unchanged.
#pragma once
#include <string>
#include <vector>

namespace sf {
struct SfLammps;

// ---- the compute (called by sf_compute_atom.hip for the style chunk/atom and for IDs it does not hold) ----
void chunk_compute_define(SfLammps& L, const std::vector<std::string>& w);
bool chunk_compute_exists(const SfLammps& L, const std::string& id);
void chunk_compute_remove(SfLammps& L, const std::string& id);
// the chunk IDs as doubles, one per owned atom (0: outside the group, or discarded), assigned once per step
const double* chunk_compute_values(SfLammps& L, const std::string& id);
void chunk_invalidate(SfLammps& L);

// ---- the fix ----
// `fix ID group ave/chunk ...` from the whole line (its title keywords may be quoted)
void ave_chunk_fix_command(SfLammps& L, const std::string& line);
bool ave_chunk_fix_exists(const SfLammps& L, const std::string& id);
// `unfix ID`: a fix ave/chunk, a fix ave/time (sf_global.hip) or a fix ave/histo (sf_histo.hip)
void unfix_command(SfLammps& L, const std::vector<std::string>& w);
// does a fix ave/chunk name this compute (as its chunk compute or as a c_ value)?
bool ave_chunk_uses_compute(const SfLammps& L, const std::string& id);

// ---- the run (sf::run_steps) ----
bool ave_chunk_active(const SfLammps& L);
// the first step after `step` at which some fix ave/chunk samples (-1: none)
long long ave_chunk_next_step(const SfLammps& L, long long step);
// the samples (and outputs) due at the engine's current step that were not taken yet
void ave_chunk_sample_due(SfLammps& L);
}  // namespace sf
