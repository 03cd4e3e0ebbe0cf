// sf_handles.h -- what the opaque `void* ptr` of the sf_lammps_* / sf_dem_* C-ABI points to, and the small helpers every
// file behind that ABI needs: handle(), refuse_decomposed(), stream_ms().
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "sf_dem.h"

namespace sf {
struct SfLammps {
  DemEngine eng;
  bool pair_hybrid = false;
  intptr_t comm = 0;
  // The world the LAMMPS object was opened on (sf_lammps_open_world <- `new LAMMPS(0, NULL, commLammps)` on a
  // duplicated world communicator, lammpsFoam/softParticleCloud.C:60-62).  With more than one rank the engine
  // decomposes ITSELF the way LAMMPS does: `processors px py pz` -> a grid of bricks when the box is created
  // (read_data), every later lammps_* call collective (interfaceToLammps/library.cpp:94-131,372-386).
  int world_rank = 0, world_size = 1;
  char comm_id[128] = {0};       // RCCL unique id of rank 0, broadcast by the caller's MPI
  int procgrid[3] = {0, 0, 0};   // `processors px py pz`, 0 = `*` ([3P] LAMMPS chooses by surface area)
  bool decomposed = false;       // the bricks were set up by the script path (sf_brick_init behind read_data)
  bool pending_rebuild = false;  // lammps_create_particle / lammps_delete_particle: next_reneighbor (library.cpp:482-486)
  long long natoms = -1;         // atom->natoms (library.cpp:94-98): set by read_data, create / delete particle
  std::vector<std::string> property_atom_ids;   // IDs of `fix ID all property/atom mol` (read_data ... fix ID NULL Molecules)
  // RCCL communicator + events of the C++ halo loop (sf_halo_rccl.hip); opaque here so that only that file
  // sees the RCCL headers
  void* halo = nullptr;
  void (*halo_delete)(void*) = nullptr;
  // the `dump` commands and their writer thread (sf_dump.hip); opaque here like halo
  void* dumps = nullptr;
  void (*dumps_delete)(void*) = nullptr;
  // thermo settings, destinations and the last line (sf_thermo.hip); opaque here like halo
  void* thermo = nullptr;
  void (*thermo_delete)(void*) = nullptr;
  // the `restart` schedule, the fix IDs of the walls and the wall rows of a restart file (sf_restart.hip); opaque like halo
  void* restart = nullptr;
  void (*restart_delete)(void*) = nullptr;
  // the `compute pair/local` commands and the device scratch of their rows (sf_contacts.hip); opaque like halo
  void* computes = nullptr;
  void (*computes_delete)(void*) = nullptr;
  // the per-atom computes and their device buffers (sf_compute_atom.hip); opaque like halo
  void* atom_computes = nullptr;
  void (*atom_computes_delete)(void*) = nullptr;
  // the chunk/atom computes, the fix ave/chunk commands, their device buffers and files (sf_chunk.hip); opaque like halo
  void* chunks = nullptr;
  void (*chunks_delete)(void*) = nullptr;
  // the global computes, the fix ave/time commands, their device values, accumulators and files (sf_global.hip); opaque like halo
  void* globals = nullptr;
  void (*globals_delete)(void*) = nullptr;
  // the fix ave/histo commands, their device counters and files (sf_histo.hip); opaque like halo
  void* histos = nullptr;
  void (*histos_delete)(void*) = nullptr;
  // the device scratch of the image-count query and of the tags lammps_create_particle tells the displacement computes about
  // (sf_displace.hip); opaque like halo
  void* displace = nullptr;
  void (*displace_delete)(void*) = nullptr;
  // the regions, the dynamic groups, their programs and member counts on the device (sf_region.hip); opaque like halo
  void* regions = nullptr;
  void (*regions_delete)(void*) = nullptr;
  // the compute rdf commands, the cutoff grids and their device buffers (sf_nbr.hip); opaque like halo
  void* nbr = nullptr;
  void (*nbr_delete)(void*) = nullptr;
  ~SfLammps()
  {
    if (regions && regions_delete) regions_delete(regions);
    if (displace && displace_delete) displace_delete(displace);
    if (restart && restart_delete) restart_delete(restart);
    if (thermo && thermo_delete) thermo_delete(thermo);   // (closes the log and screen files)
    if (dumps && dumps_delete) dumps_delete(dumps);   // (drains the writer: the frames are in their files)
    if (histos && histos_delete) histos_delete(histos);   // (closes the files of fix ave/histo)
    if (globals && globals_delete) globals_delete(globals);   // (closes the files of fix ave/time)
    if (chunks && chunks_delete) chunks_delete(chunks);   // (closes the files of fix ave/chunk; after the dumps, like computes)
    if (computes && computes_delete) computes_delete(computes);   // (after the dumps, whose frames read its rows)
    if (atom_computes && atom_computes_delete) atom_computes_delete(atom_computes);   // (likewise)
    if (nbr && nbr_delete) nbr_delete(nbr);   // (after the fixes ave/time, whose samples read its arrays)
    if (halo && halo_delete) halo_delete(halo);
  }
};

inline SfLammps* handle(void* p)
{
  if (!p) fail("null engine handle");
  return static_cast<SfLammps*>(p);
}

// the GPU milliseconds of what `work` puts on stream `s`, between two events (waits for the stream)
template <class Work>
double stream_ms(hipStream_t s, Work&& work)
{
  struct Events {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~Events()
    {
      for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    }
  } E;
  for (hipEvent_t& e : E.ev) SF_HIP(hipEventCreate(&e));
  SF_HIP(hipEventRecord(E.ev[0], s));
  work();
  SF_HIP(hipEventRecord(E.ev[1], s));
  SF_HIP(hipStreamSynchronize(s));
  float ms = 0.f;
  SF_HIP(hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
  return (double)ms;
}

// what reads the whole bed from one device refuses a decomposed run; `who` as in "fix ave/chunk"
inline void refuse_decomposed(const SfLammps& L, const char* who)
{
  const DemEngine& e = L.eng;
  if (L.world_size > 1 || L.decomposed || e.nranks() > 1 || e.decomposed())
    fail("%s: one rank only (no decomposed domain)", who);
}
}  // namespace sf
