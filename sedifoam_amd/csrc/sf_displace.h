// sf_displace.h -- what the unwrapped-coordinate keywords share: the view of the engine's image
// table an evaluation kernel takes, and the table of reference positions of a displacement compute.  sf_displace.hip
// holds the code; compute displace/atom lives in sf_compute_atom.hip, compute com in sf_global.hip.
#pragma once
#include <string>
#include <vector>

#include "sf_handles.h"
#include "sf_unmap.h"

namespace sf {

// The image table as it is now, for a keyword `who` (as in "compute com").  Refused on more than one rank (there the
// migration shift wraps, uncounted), with fix rigid/nve (the rigid integrator places the atoms itself), and on an engine
// that has wrapped atoms before any keyword asked for the counts.  The first keyword of an engine makes the table.
ImageView image_view(SfLammps& L, const char* who);

// The reference positions of one displacement compute: the unwrapped position of every tag at the moment the compute was
// defined (of an atom created later: at its creation), row tag of [rows][3]; owned by the compute.
struct RefTable {
  double* x0 = nullptr;
  size_t rows = 0;
  RefTable() = default;
  RefTable(const RefTable&) = delete;
  RefTable& operator=(const RefTable&) = delete;
  ~RefTable();
  void fit(DemEngine& e);   // rows for every tag up to max_tag(), the old rows kept
};

// x0[tag] = unmap(x) for every owned atom.  One launch
void ref_set_all(SfLammps& L, RefTable& R, const ImageView& V);
// the same for the atoms with the tags d_tags[0 .. np) only.  Two launches, no host round trip
void ref_set_tags(SfLammps& L, RefTable& R, const ImageView& V, const int* d_tags, int np);

// lammps_create_particle has made atoms with these tags: every displacement compute takes where they are now as their
// reference (atom_compute_created)
void displace_created(SfLammps& L, const double* tags, int np);

}  // namespace sf
