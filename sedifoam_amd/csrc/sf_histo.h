// sf_histo.h -- `fix ID group ave/histo Nevery Nrepeat Nfreq lo hi Nbin value ...` (sf_histo.hip): the distribution of
// per-atom values, of the columns of a compute pair/local or of global values, counted into bins on the GPU, accumulated
// over time and written as a histogram.  The fix shares the ID space of fix ave/chunk and fix
// ave/time (sf_ave_fix.h, which also has `unfix` and the run's cuts).
#pragma once
#include <string>
#include <vector>

namespace sf {
struct SfLammps;

// `fix ID group ave/histo ...` from the whole line (its title keywords may be quoted)
void ave_histo_fix_command(SfLammps& L, const std::string& line);

// ---- the run (ave_fix_step_due of sf_ave_fix.hip) ----
// the global computes that the samples due at the engine's current step bin, added to `ids`: they join the plan of
// global_step_due (sf_global.hip), which runs before ave_histo_sample_due, so that each is evaluated once
void ave_histo_global_ids_due(SfLammps& L, std::vector<std::string>* ids);
// the samples (and outputs) due at the engine's current step that were not taken yet
void ave_histo_sample_due(SfLammps& L);
}  // namespace sf
