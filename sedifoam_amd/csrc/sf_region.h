// sf_region.h -- `region`, `group ID region`, `group ID dynamic ... region ... every N` and `group ID static` (DESIGN.md
// section 18): what sf_lammps_api.hip calls.  sf_region.hip holds the table, the kernels and the C-ABI queries;
// sf_region_parse.h the words, sf_region_match.h the predicate.
#pragma once
#include <string>
#include <vector>

#include "sf_handles.h"

namespace sf {

// w = region ID style args ... | region ID delete
void region_command(SfLammps& L, const std::vector<std::string>& w);
// w = group ID region RID: the atoms of the region are added to the group, evaluated once, now
void group_region_command(SfLammps& L, const std::vector<std::string>& w);
// w = group ID dynamic PARENT region RID [every N]: assigns nothing; the next evaluation does
void group_dynamic_command(SfLammps& L, const std::vector<std::string>& w);
// w = group ID static: the membership as it stands is kept
void group_static_command(SfLammps& L, const std::vector<std::string>& w);
bool group_is_dynamic(const SfLammps& L, const std::string& name);

// a fix the sub-step kernel or the rigid integrator implements decides its group bit once: refused on a dynamic group,
// before the fix is made.  (The converse, `group G dynamic` on a group such a fix uses, asks the engine:
// DemEngine::fix_uses_group_bit)
void region_refuse_engine_fix(const SfLammps& L, const std::string& style, const std::string& group);
// read_restart replaces the engine's groups: refused while a dynamic group exists
bool region_dynamic_any(const SfLammps& L);

// ---- the run (sf::run_steps) ----
// the first step after `step` that is a multiple of some dynamic group's N; -1: there is no dynamic group
long long region_next_step(const SfLammps& L, long long step);
// the setup of a `run` command evaluates every dynamic group (run_steps does it: region_begin_due)
void region_run_setup(SfLammps& L);
// the beginning of a piece of running: the groups a `run` has marked, and those not evaluated since their definition
void region_begin_due(SfLammps& L);
// the end of a step: the groups whose N divides it, in one launch
void region_step_due(SfLammps& L);

}  // namespace sf
