// sf_dump.h -- `dump ID group custom N file attr...`, `dump_modify ID sort id`, `undump ID` (sf_dump.hip): the
// particle snapshots of the reference's input scripts, formatted on the GPU.
#pragma once
#include <string>
#include <vector>

namespace sf {
struct SfLammps;

void dump_command(SfLammps& L, const std::vector<std::string>& w);
void dump_modify_command(SfLammps& L, const std::vector<std::string>& w);
void undump_command(SfLammps& L, const std::vector<std::string>& w);
bool dump_active(const SfLammps& L);
// the first step after `step` at which some dump writes a frame (-1: none)
long long dump_next_step(const SfLammps& L, long long step);
// the frames due at the engine's current step that were not written yet ([3P] Output::setup / Output::write)
void dump_write_due(SfLammps& L);
// wait until the writer has put every queued frame into its file (rethrows a write error)
void dump_drain(SfLammps& L);
// "run n pre no post no" with the frames of the active dumps (sf_lammps_api.hip): lammps_step, the script's `run` and
// the cloud's DEM sub-cycles
void run_steps(SfLammps& L, int n);
// (sf_halo_rccl.hip, collective) every rank's nbytes at src (device) after one another in rank order in rank 0's *dst
// (device, grown as needed: capacity *cap); returns the total byte count on rank 0, and the sum of count on every rank
size_t dump_gather(SfLammps& L, const char* src, size_t nbytes, unsigned long long count, char** dst, size_t* cap,
                   unsigned long long* count_total);
}  // namespace sf
