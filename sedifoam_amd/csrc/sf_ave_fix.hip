// sf_ave_fix.hip -- the registry of the averaging fixes (sf_ave_fix.h): the one place that lists the kinds.
#include "sf_ave_fix.h"

#include <array>

#include "sf_chunk.h"
#include "sf_global.h"
#include "sf_histo.h"

namespace sf {
namespace {
// in the order in which the kinds sample within a step (ave_fix_step_due)
std::array<const AveFixKind*, 3> kinds() { return {{&ave_chunk_kind(), &ave_time_kind(), &ave_histo_kind()}}; }
}  // namespace

bool ave_fix_exists(const SfLammps& L, const std::string& id)
{
  for (const AveFixKind* k : kinds())
    if (k->exists(L, id)) return true;
  return false;
}

void unfix_command(SfLammps& L, const std::vector<std::string>& w)
{
  if (w.size() != 2) fail("Illegal unfix command");
  for (const AveFixKind* k : kinds())
    if (k->unfix(L, w[1])) return;
  fail("unfix %s: only a fix ave/chunk can be removed (or a fix ave/time or ave/histo), and there is none with this ID (the other fixes "
       "stay for the whole script)", w[1].c_str());
}

const char* ave_fix_uses_compute(const SfLammps& L, const std::string& id)
{
  for (const AveFixKind* k : kinds())
    if (k->uses_compute(L, id)) return k->style;
  return nullptr;
}

long long ave_fix_next_step(const SfLammps& L, long long step)
{
  long long best = -1;
  for (const AveFixKind* k : kinds()) {
    const long long nx = k->next_step(L, step);
    if (nx >= 0 && (best < 0 || nx < best)) best = nx;
  }
  return best;
}

void ave_fix_step_due(SfLammps& L, std::vector<std::string> global_ids)
{
  ave_chunk_sample_due(L);
  ave_histo_global_ids_due(L, &global_ids);
  global_step_due(L, global_ids);
  ave_histo_sample_due(L);
}

}  // namespace sf
