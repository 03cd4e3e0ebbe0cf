// sf_compute_ids.hip -- the registry of the computes (sf_compute_ids.h): the one place that lists the kinds.
#include "sf_compute_ids.h"

#include <array>

#include "sf_ave_fix.h"
#include "sf_chunk.h"
#include "sf_contacts.h"
#include "sf_global.h"
#include "sf_pchunk.h"
#include "sf_thermo.h"

namespace sf {
namespace {
std::array<const ComputeKindOps*, 5> kinds()
{
  return {{&pair_local_kind(), &atom_compute_kind(), &global_compute_kind(), &rdf_compute_kind(), &pchunk_compute_kind()}};
}

// the kind that holds compute `id` and the compute's shape; nullptr: no compute has this ID
const ComputeKindOps* owner_of(const SfLammps& L, const std::string& id, ComputeShape* s)
{
  for (const ComputeKindOps* k : kinds())
    if (k->shape(L, id, s)) return k;
  *s = ComputeShape();
  return nullptr;
}
}  // namespace

ComputeShape compute_shape(const SfLammps& L, const std::string& id)
{
  ComputeShape s;
  owner_of(L, id, &s);
  return s;
}

void computes_invalidate(SfLammps& L)
{
  for (const ComputeKindOps* k : kinds()) k->invalidate(L);
  chunk_invalidate(L);   // (chunk/atom is defined and removed through sf_compute_atom.hip; its stamps are its own)
}

// compute ID group-ID STYLE ...  |  uncompute ID
bool compute_command(SfLammps& L, const std::vector<std::string>& w)
{
  if (w[0] == "uncompute") {
    if (w.size() != 2) fail("Illegal uncompute command");
    const std::string& id = w[1];
    ComputeShape shape;
    const ComputeKindOps* owner = owner_of(L, id, &shape);
    const ComputeKind kind = shape.kind;
    if (!owner) fail("Could not find compute ID to delete");   // [3P] Modify::delete_compute
    if (reduce_uses_compute(L, id)) fail("uncompute %s: a compute reduce still uses this compute (uncompute it first)", id.c_str());
    if (const char* who = pchunk_uses_compute(L, id))
      fail("uncompute %s: a %s still uses this compute (uncompute it first)", id.c_str(), who);
    if (const char* who = ave_fix_uses_compute(L, id))
      fail("uncompute %s: a %s still uses this compute (unfix it first)", id.c_str(), who);
    if (kind == CK_GLOBAL && thermo_uses_compute(L, id))
      fail("uncompute %s: thermo_style custom still names this compute (give another thermo_style first)", id.c_str());
    if ((kind == CK_PERATOM || kind == CK_LOCAL) && dump_uses_compute(L, id))
      fail("uncompute %s: a dump %s still uses this compute (undump it first)", id.c_str(), kind == CK_PERATOM ? "custom" : "local");
    owner->remove(L, id);
    return true;
  }
  if (w[0] != "compute") return false;
  if (w.size() < 4) fail("Illegal compute command");
  const std::string& style = w[3];
  if (style == "cohe/local")
    fail("compute cohe/local is not built (fix cohesive is a fix and has no single(); the reference's own code behind it "
         "never terminates)");
  const ComputeKindOps* owner = nullptr;
  for (const ComputeKindOps* k : kinds())
    if (k->is_style(style)) owner = k;
  if (!owner)
    fail("Invalid compute style %s (this engine has compute pair/local, also under the name gran/local, the per-atom "
         "computes stress/atom, contact/atom, ke/atom, erotate/sphere/atom, property/atom and chunk/atom, and the global "
         "computes reduce, ke and erotate/sphere; on unwrapped coordinates the per-atom compute displace/atom and the global "
         "compute com; on a grid of the user's cutoff the global array rdf and the per-atom computes coord/atom and cluster/atom, and "
         "the global compute cluster/stats; over the chunks of a compute chunk/atom c_ID the global arrays property/chunk, "
         "com/chunk, vcm/chunk and gyration/chunk)", style.c_str());
  (void)L.eng.group_bit(w[2]);   // (the group must exist, before the ID is looked at)
  if (compute_shape(L, w[1]).kind != CK_NONE) fail("Reuse of compute ID");
  owner->define(L, w);
  return true;
}

}  // namespace sf
