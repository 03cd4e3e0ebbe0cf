// sf_global.h -- the global computes `compute ID group reduce MODE input ...`, `compute ID group ke` and `compute ID group
// erotate/sphere`, and `fix ID group ave/time Nevery Nrepeat Nfreq c_ID ...` (sf_global.hip): one number per step that the
// user chooses, reduced over the whole bed on the GPU and written as a time series.  The computes share the ID space of the
// other computes (sf_compute_ids.h: they plug in there as global_compute_kind()); the fix shares the ID space of the other
// averaging fixes (sf_ave_fix.h).
#pragma once
#include <string>
#include <vector>

namespace sf {
struct SfLammps;

// ---- the computes ----
// is global compute `id` extensive (thermo divides such a value by the atom count under norm yes)?
bool global_compute_extensive(const SfLammps& L, const std::string& id);
// does a compute reduce name compute `id` as an input?
bool reduce_uses_compute(const SfLammps& L, const std::string& id);
// the values of `id` on the state as it stands, on the host (evaluated first when they are stale; one copy, one wait)
void global_values_host(SfLammps& L, const std::string& id, std::vector<double>* out);
// ... and where they lie on the device (evaluated first when they are stale; no copy, no wait): nvalues doubles that stay
// at this address while the compute exists (fix ave/histo bins them there, sf_histo.hip)
const double* global_values_device(SfLammps& L, const std::string& id);

// ---- the fix (its ID space, unfix and the run's cuts: sf_ave_fix.h) ----
// `fix ID group ave/time ...` from the whole line (its title keywords may be quoted)
void ave_time_fix_command(SfLammps& L, const std::string& line);

// ---- the run (ave_fix_step_due of sf_ave_fix.hip) ----
// One evaluation plan for the engine's current step: the computes of the fix ave/time samples due now and those named in
// `also` (the c_ columns of a thermo line due now, the global inputs of the fix ave/histo samples due now), each evaluated
// once; then the samples and outputs of the fixes
void global_step_due(SfLammps& L, const std::vector<std::string>& also);
}  // namespace sf
