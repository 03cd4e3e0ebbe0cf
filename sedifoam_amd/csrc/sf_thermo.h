// sf_thermo.h -- thermo output of the LAMMPS-shaped surface (sf_thermo.hip): `thermo N`, `thermo_style one | custom`,
// `thermo_modify norm | flush | lost error`, `units`, `log`, `echo`, and the -screen / -log arguments of
// sf_lammps_open.  The whole-bed sums behind a line (kinetic tensor, pair virial, force norms) are reduced on the GPU.
#pragma once
#include <string>
#include <vector>

#include "sf_dem.h"

namespace sf {
struct SfLammps;

// ---- script surface ----
// -screen / -log of argv (LAMMPS' own parsing starts at argv[1]), then the SF_SCREEN / SF_LOG knobs for what argv left
// unset.  Both default to none.
void thermo_open_args(SfLammps& L, int argc, char** argv);
// the commands this file owns; false: not one of them
bool thermo_command(SfLammps& L, const std::vector<std::string>& w);
// an input line as LAMMPS echoes it (Input::file / Input::one, `echo` setting)
void thermo_echo(SfLammps& L, const std::string& line);
// `units lj | si`: boltz and the default of `norm`
void thermo_units(SfLammps& L, bool lj);
bool thermo_units_lj(const SfLammps& L);   // (what a checkpoint records)
// the `timestep` command, before dt changes: atime += (step - atimestep) dt ([3P] Update::update_time)
void thermo_update_time(SfLammps& L);

// ---- the run (sf::run_steps) ----
// a destination is open: lines are computed and written.  The same answer on every rank (rank 0 alone writes).
bool thermo_active(const SfLammps& L);
// a line of the current style shows a quantity that counts degrees of freedom (temp, press, ke, etotal, p**)
bool thermo_needs_dof(const SfLammps& L);
// before the setup of a run: arm the pair virial of the setup force evaluation (first run only)
void thermo_run_begin(SfLammps& L);
// header and the line of the setup; `n` = steps of the run
void thermo_setup(SfLammps& L, int n);
// the first step after `step` at which a line is written inside the current run (the run's last step included)
long long thermo_next_step(const SfLammps& L, long long step);
// arm the virial pass for a piece of the run that ends at step `end`
void thermo_arm(SfLammps& L, long long end);
// the line of the current step if it is due (a multiple of N or the run's last step)
void thermo_write_due(SfLammps& L);
// `Loop time of ...`
void thermo_run_end(SfLammps& L);

// the value of `keyword` in the last line written: 0, -1 when no line was written yet, -2 for an unknown keyword
int thermo_get(const SfLammps& L, const std::string& keyword, double* out);
// the global computes the c_ID / c_ID[k] columns of the current style name (sf_global.hip evaluates them): those of the
// line due at the engine's current step -- at the setup of a run (`setup`), at a multiple of N or at the run's last step --
// or nothing when no line is due or no destination is open
std::vector<std::string> thermo_global_ids_due(const SfLammps& L, bool setup, int run_n);
// does the current thermo style name compute `id`?
bool thermo_uses_compute(const SfLammps& L, const std::string& id);
// kernel launches made for thermo output so far (the virial pass and the reductions)
long long thermo_launches(const SfLammps& L);

// ---- device side (sf_thermo.hip), called by DemEngine::launch_substep ----
// k_thermo_virial over the owned atoms of the launch described by P, S: per-block partials of sum 1/2 del (x) F_pair
// (6 components, LAMMPS order xx yy zz xy xz yz) into out[6 * nblocks]
int thermo_virial_blocks(int nlocal);
void thermo_virial_launch(const DemPtrs& P, const StepParams& S, bool lub, double* out, int nblocks, hipStream_t s);
}  // namespace sf
