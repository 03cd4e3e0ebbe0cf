// sf_restart.h -- checkpoints (sf_restart.hip): `write_restart FILE`, `restart N ...`, `read_restart FILE`.  The file
// format (version 1) is specified by sedifoam_amd/restart.py, which writes and reads the same bytes; DESIGN.md section 10.
#pragma once
#include <string>
#include <utility>
#include <vector>

namespace sf {
struct SfLammps;

struct RestartWall {
  std::string id;               // the fix ID
  std::vector<int> tag;         // atoms whose touch bit is set for this wall, ascending
  std::vector<double> shear;    // [3][m]
};

// host image of a checkpoint: the columns of the file, atoms in ascending tag order
struct RestartData {
  long long natoms = 0, ncontacts = 0, step = 0, max_tag = 0;
  double dt = 0.0, lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
  int periodic[3] = {0, 0, 0}, units_lj = 1;
  std::vector<std::pair<std::string, int>> groups;   // ascending bit
  std::vector<int> tag, type, mask, foam, ccount, cpartner;
  std::vector<double> x, radius, v, rmass, omega, fdrag, DuDt, vOld, cshear;   // [3][n] / [n] / [3][nc]
  std::vector<RestartWall> walls;
};

// FILE.tmp, flush, rename; every failure is an sf::Error
void restart_file_write(const std::string& path, const RestartData& d);
void restart_file_read(const std::string& path, RestartData& d);

// ---- script surface (sf_lammps_api.hip) ----
void restart_command(SfLammps& L, const std::vector<std::string>& w);
void write_restart_command(SfLammps& L, const std::string& file);
// what read_restart keeps for the fix lines that follow: the saved wall rows, claimed by fix ID
void restart_set_pending_walls(SfLammps& L, std::vector<RestartWall>&& walls);
// a `fix ID group wall/gran...` line registered engine wall `w`: remember its ID; restore the rows a restart file saved for it
void restart_fix_wall(SfLammps& L, const std::string& id, int w);
// ---- the run (sf::run_steps) ----
bool restart_active(const SfLammps& L);
// saved wall state that no fix has claimed is dropped (and the log says so)
void restart_run_begin(SfLammps& L);
long long restart_next_step(const SfLammps& L, long long step);   // the first checkpoint step after `step`
void restart_write_due(SfLammps& L);
long long restart_launches(const SfLammps& L);
// wait until the writer thread has put every queued checkpoint into its file; a write error is thrown here
void restart_drain(SfLammps& L);
// the blocks of DemEngine::restart_pack_device of one or more ranks -> the file's columns in ascending tag order
void restart_blocks_to_data(const char* host, size_t nbytes, RestartData& d);
// cost of the last checkpoint (tools/restart_cost.py): {GPU ms of the pack, host ms until the pinned copy has landed,
// host ms until the file was renamed, 0}; timing on: the pack is bracketed by events and waited for
void restart_timing(SfLammps& L, bool on);
void restart_last_cost(SfLammps& L, double out[4]);   // kernel launches made for checkpoints so far
}  // namespace sf
