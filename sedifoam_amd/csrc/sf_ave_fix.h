// sf_ave_fix.h -- the one ID space of fix ave/chunk (sf_chunk.hip), fix ave/time (sf_global.hip) and fix ave/histo
// (sf_histo.hip), and what the three keep alike on the engine's side: the state of the latest output and its file, and the
// helpers over a set's list of fixes.  The registry is sf_ave_fix.hip; a kind plugs in with one AveFixKind.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "sf_ave_common.h"
#include "sf_handles.h"

namespace sf {

// ---- the registry ----
// is `id` the ID of an averaging fix of any kind?
bool ave_fix_exists(const SfLammps& L, const std::string& id);
// `unfix ID`
void unfix_command(SfLammps& L, const std::vector<std::string>& w);
// the style ("fix ave/chunk", ...) of an averaging fix that names compute `id`, or nullptr
const char* ave_fix_uses_compute(const SfLammps& L, const std::string& id);
// the first step after `step` at which some averaging fix samples; -1: there is none (sf::run_steps cuts the run there)
long long ave_fix_next_step(const SfLammps& L, long long step);
// The samples (and outputs) due at the engine's current step that were not taken yet, in this order: every fix ave/chunk;
// one plan of global computes -- those of the fix ave/time samples, those in `global_ids` (the c_ columns of a thermo line
// due now) and the global inputs of the fix ave/histo samples, each evaluated once; every fix ave/histo
void ave_fix_step_due(SfLammps& L, std::vector<std::string> global_ids);

// ---- what a kind gives the registry ----
struct AveFixKind {
  const char* style;
  bool (*exists)(const SfLammps& L, const std::string& id);
  bool (*unfix)(SfLammps& L, const std::string& id);   // false: no fix of this kind has this ID
  bool (*uses_compute)(const SfLammps& L, const std::string& id);
  long long (*next_step)(const SfLammps& L, long long step);
};
const AveFixKind& ave_chunk_kind();   // (sf_chunk.hip)
const AveFixKind& ave_time_kind();    // (sf_global.hip)
const AveFixKind& ave_histo_kind();   // (sf_histo.hip)

// ---- what a fix of any kind holds besides its spec S (an AveSchedule with an id) and its accumulator ----
struct AveFixState {
  AveFile file;
  bool have = false;   // the latest output
  long long out_step = -1;
};

template <class F>
F* ave_find(const std::vector<std::unique_ptr<F>>& fixes, const std::string& id)
{
  for (auto& f : fixes)
    if (f->S.id == id) return f.get();
  return nullptr;
}

// fix `id` taken out of the list once nothing queued on the stream can still add into its accumulator (destroying it closes
// its file); nullptr: no such fix
template <class F>
std::unique_ptr<F> ave_take(SfLammps& L, std::vector<std::unique_ptr<F>>& fixes, const std::string& id)
{
  for (size_t k = 0; k < fixes.size(); k++)
    if (fixes[k]->S.id == id) {
      SF_HIP(hipStreamSynchronize(L.eng.stream()));
      std::unique_ptr<F> f = std::move(fixes[k]);
      fixes.erase(fixes.begin() + k);
      return f;
    }
  return nullptr;
}

template <class F>
long long ave_next(const std::vector<std::unique_ptr<F>>& fixes, long long step)
{
  long long best = -1;
  for (const auto& f : fixes) {
    const long long nx = f->S.next(step);
    if (best < 0 || nx < best) best = nx;
  }
  return best;
}

}  // namespace sf
