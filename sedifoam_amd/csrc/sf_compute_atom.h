// sf_compute_atom.h -- the per-atom computes `compute ID group stress/atom | contact/atom | ke/atom | erotate/sphere/atom |
// property/atom | displace/atom | coord/atom | cluster/atom` (sf_compute_atom.hip): one value (stress/atom: six; property/atom: one per attribute) per owned atom, evaluated on the GPU from the state at the moment of
// the output, behind the `c_ID` / `c_ID[k]` columns of `dump custom` (sf_dump.hip) and sf_lammps_compute_atom.  They share
// the ID space of the other computes: sf_compute_ids.h owns `compute` / `uncompute`, and these styles (chunk/atom of
// sf_chunk.hip among them, forwarded) plug in there as atom_compute_kind().
#pragma once
#include <string>
#include <vector>

#include "sf_nbr.h"

namespace sf {

// The values of compute `id` on the state as it stands, field-major on the device: column c of atom index i at
// [c * nlocal + i]; atoms outside the compute's group hold 0.  Evaluated once per step however many dumps and queries
// ask: the buffer is kept with the step (and the rebuild and atom counts) it was made at, on the engine's stream.
const double* atom_compute_values(SfLammps& L, const std::string& id, int* ncols);
long long atom_compute_launches(const SfLammps& L);
// GPU time from HIP events of one fresh evaluation of `id` (tools/compute_atom_cost.py)
double atom_compute_cost(SfLammps& L, const std::string& id);
// compute coord/atom `id`: its group bit, cutoff and type ranges (sf_lammps_nbr_cost times its grid and walk); false: no
// compute coord/atom has this ID
bool atom_compute_coord_spec(const SfLammps& L, const std::string& id, int* groupbit, double* rc, std::vector<TypeRange>* ranges);
// compute cluster/atom `id`: its group bit and spec, and what it keeps between evaluations (the verify rounds of the last one
// among it; sf_lammps_nbr_cost times its grid and walk, compute cluster/stats asks whether CID is one); nullptr: no compute
// cluster/atom has this ID
ClusterWork* atom_compute_cluster_spec(const SfLammps& L, const std::string& id, int* groupbit, ClusterSpec* spec);
// compute displace/atom: is there one, and lammps_create_particle has made atoms with the tags d_tags[0 .. np) (device) --
// where they are now is their reference (displace_created of sf_displace.hip calls both)
bool atom_compute_tracks_created(const SfLammps& L);
void atom_compute_created(SfLammps& L, const int* d_tags, int np);
}  // namespace sf
