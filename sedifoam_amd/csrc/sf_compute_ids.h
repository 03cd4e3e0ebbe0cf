// sf_compute_ids.h -- the one ID space of the computes: compute pair/local (sf_contacts.hip), the per-atom computes
// (sf_compute_atom.hip, which forwards chunk/atom to sf_chunk.hip), the global computes (sf_global.hip), compute rdf
// (sf_nbr.hip) and the per-chunk computes (sf_pchunk.hip).  The registry is sf_compute_ids.hip: it owns `compute` / `uncompute`, answers what an ID is, and tells every
// owner that the state changed.  A kind plugs in with one ComputeKindOps.  What a reader of c_ID then accepts: sf_compute_ref.h.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "sf_compute_ref.h"
#include "sf_handles.h"

namespace sf {

// ---- the registry ----
// what compute `id` is (kind CK_NONE: no compute has this ID)
ComputeShape compute_shape(const SfLammps& L, const std::string& id);
// `compute ID group STYLE ...` | `uncompute ID`: true when the word was one of the two
bool compute_command(SfLammps& L, const std::vector<std::string>& w);
// the state changed at an unchanged step (a script command, atoms created or deleted, a group's members): every compute is
// evaluated again when asked next
void computes_invalidate(SfLammps& L);

// ---- what a kind gives the registry ----
struct ComputeKindOps {
  bool (*is_style)(const std::string& style);
  void (*define)(SfLammps& L, const std::vector<std::string>& w);   // (the registry has checked that the ID is new)
  void (*remove)(SfLammps& L, const std::string& id);
  bool (*shape)(const SfLammps& L, const std::string& id, ComputeShape* s);   // false: no compute of this kind has this ID
  void (*invalidate)(SfLammps& L);
};
const ComputeKindOps& pair_local_kind();       // (sf_contacts.hip)
const ComputeKindOps& atom_compute_kind();     // (sf_compute_atom.hip)
const ComputeKindOps& global_compute_kind();   // (sf_global.hip)
const ComputeKindOps& rdf_compute_kind();      // (sf_nbr.hip)
const ComputeKindOps& pchunk_compute_kind();   // (sf_pchunk.hip: property/chunk, com/chunk, vcm/chunk, gyration/chunk)

// compute `id` taken out of an owner's list once nothing queued on the stream can still read or write its buffers;
// nullptr: no such compute
template <class C>
std::unique_ptr<C> compute_take(SfLammps& L, std::vector<std::unique_ptr<C>>& computes, const std::string& id)
{
  for (size_t k = 0; k < computes.size(); k++)
    if (computes[k]->id == id) {
      SF_HIP(hipStreamSynchronize(L.eng.stream()));
      std::unique_ptr<C> c = std::move(computes[k]);
      computes.erase(computes.begin() + k);
      return c;
    }
  return nullptr;
}

}  // namespace sf
