// sf_nbr.h -- the neighbourhood walk on a grid of the user's cutoff (sf_nbr.hip): who is near a grain
// without touching it.  `compute ID group rdf Nbin [itype jtype ...] cutoff Rc` (a global array) lives here; `compute ID group
// coord/atom cutoff Rc [typerange ...]` is a per-atom style of sf_compute_atom.hip whose evaluation is nbr_coord_atom.  The
// walk reads the positions as they stand and stores nothing that the run reads; compute_command (sf_contacts.hip) owns the ID
// space and hands `rdf` over.
#pragma once
#include <string>
#include <vector>

#include "sf_nbr_parse.h"

namespace sf {
struct SfLammps;

// ---- compute rdf ----
bool rdf_compute_style(const std::string& style);
// `compute ID group rdf ...` (the caller has checked that the ID is new)
void rdf_compute_define(SfLammps& L, const std::vector<std::string>& w);
// rows (Nbin) and columns (1 + 2 npairs) of the global array of compute `id`; 0: no compute rdf has this ID
int rdf_array_rows(const SfLammps& L, const std::string& id, int* ncols = nullptr);
void rdf_compute_remove(SfLammps& L, const std::string& id);
// the array on the device, row-major [rows][ncols], on the state as it stands (evaluated first when it is stale; no copy, no
// wait): it stays at this address while the compute exists (fix ave/time mode vector adds its columns there)
const double* rdf_array_device(SfLammps& L, const std::string& id);

// ---- compute coord/atom (called by sf_compute_atom.hip) ----
// column k of val (field-major, [k * nlocal + i]): the atoms j != i of any group with rsq < rc^2 and a type in ranges[k], for
// the atoms i of the group; 0 for the others.  `who` as in "compute coord/atom"
void nbr_coord_atom(SfLammps& L, const char* who, int groupbit, double rc, const std::vector<TypeRange>& ranges, double* val);
// refused at a compute line and at every evaluation: a decomposed run
void nbr_refuse_unsupported(const SfLammps& L, const char* who);

// the state changed at an unchanged step: build the grid and evaluate again when asked next (atom_compute_invalidate)
void nbr_invalidate(SfLammps& L);
}  // namespace sf
