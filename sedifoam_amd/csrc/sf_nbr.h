// sf_nbr.h -- the neighbourhood walk on a grid of the user's cutoff (sf_nbr.hip): who is near a grain
// without touching it.  `compute ID group rdf Nbin [itype jtype ...] cutoff Rc` (a global array) lives here; `compute ID group
// coord/atom cutoff Rc [typerange ...]` is a per-atom style of sf_compute_atom.hip whose evaluation is nbr_coord_atom, and
// `compute ID group cluster/atom CUT [surface no|yes] [size no|yes]` another whose evaluation is nbr_cluster_atom.  The
// walk reads the positions as they stand and stores nothing that the run reads; sf_compute_ids.h owns the ID space, and `rdf`
// plugs in there as rdf_compute_kind() (whose invalidate also forgets the grids).
#pragma once
#include <string>
#include <vector>

#include "sf_handles.h"
#include "sf_nbr_parse.h"

namespace sf {

// ---- compute rdf ----
// the global array of compute `id`, Nbin rows of 1 + 2 npairs columns, on the device, row-major [rows][ncols], on the state as it stands (evaluated first when it is stale; no copy, no
// wait): it stays at this address while the compute exists (fix ave/time mode vector adds its columns there)
const double* rdf_array_device(SfLammps& L, const std::string& id);

// ---- compute coord/atom (called by sf_compute_atom.hip) ----
// column k of val (field-major, [k * nlocal + i]): the atoms j != i of any group with rsq < rc^2 and a type in ranges[k], for
// the atoms i of the group; 0 for the others.  `who` as in "compute coord/atom"
void nbr_coord_atom(SfLammps& L, const char* who, int groupbit, double rc, const std::vector<TypeRange>& ranges, double* val);
// ---- compute cluster/atom (called by sf_compute_atom.hip) ----
// what one compute cluster/atom keeps between evaluations: the parent array, the per-root minimum tag and count and the flag
// of the verify launches (one block, grown with the bed and never freed per evaluation), and the verify rounds of the last one
struct ClusterWork {
  DeviceScratch buf;
  int rounds = 0;
};
// val[i] (and val[nlocal + i] with S.size): the smallest tag (and the atom count) of the connected component of atom i under
// the link rule of S among the atoms of the group; 0 for the others.  `who` as in "compute cluster/atom"
void nbr_cluster_atom(SfLammps& L, const char* who, int groupbit, const ClusterSpec& S, ClusterWork& W, double* val);
// the cutoff of the grid a compute cluster/atom walks: CUT, or 2 rmax + CUT with surface yes
double nbr_cluster_grid_cutoff(SfLammps& L, const ClusterSpec& S);
// refused at a compute line and at every evaluation: a decomposed run
void nbr_refuse_unsupported(const SfLammps& L, const char* who);
}  // namespace sf
