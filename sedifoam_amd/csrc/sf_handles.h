// sf_handles.h -- what the opaque `void* ptr` of the sf_lammps_* / sf_dem_* C-ABI points to, and the small helpers every
// file behind that ABI needs: handle(), refuse_decomposed(), stream_ms(), fail_if(); OpaqueSlot, DeviceScratch, StateStamp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "sf_dem.h"

namespace sf {
// One member of SfLammps whose type only its owning file knows: made on first use, deleted with the engine.
struct OpaqueSlot {
  void* p = nullptr;
  void (*del)(void*) = nullptr;
  OpaqueSlot() = default;
  OpaqueSlot(const OpaqueSlot&) = delete;
  OpaqueSlot& operator=(const OpaqueSlot&) = delete;
  ~OpaqueSlot() { reset(); }
  explicit operator bool() const { return p != nullptr; }
  template <class T>
  T* get() const { return static_cast<T*>(p); }
  template <class T>
  T& ensure()
  {
    if (!p) {
      p = new T();
      del = [](void* q) { delete static_cast<T*>(q); };
    }
    return *get<T>();
  }
  void reset()
  {
    if (p) del(p);
    p = nullptr;
  }
};

// Device scratch that only grows, geometrically: no allocation per frame, sample or evaluation once it has grown.  `s` is
// the stream whose queued work may still read the old block
struct DeviceScratch {
  void* p = nullptr;
  size_t n = 0;
  DeviceScratch() = default;
  DeviceScratch(const DeviceScratch&) = delete;
  DeviceScratch& operator=(const DeviceScratch&) = delete;
  void* get(size_t need, hipStream_t s)
  {
    if (need > n) {
      if (p) {
        SF_HIP(hipStreamSynchronize(s));
        SF_HIP(hipFree(p));
      }
      n = need + need / 4 + 4096;
      SF_HIP(hipMalloc(&p, n));
    }
    return p;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  ~DeviceScratch()
  {
    if (p) (void)hipFree(p);
  }
};

// What a cached result was made at: the step, the rebuild count and the owned-atom count.  clear() forgets the step alone,
// like the `step = -1` it replaces
struct StateStamp {
  long long step = -1, nbuilds = -1;
  int nlocal = -1;
  bool is_now(const DemEngine& e) const { return step == e.nsteps() && nbuilds == e.nbuilds() && nlocal == e.nlocal(); }
  void set(const DemEngine& e)
  {
    step = e.nsteps();
    nbuilds = e.nbuilds();
    nlocal = e.nlocal();
  }
  void clear() { step = -1; }
};

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
  // What the files behind the ABI keep per engine, each type known to its owning file alone.  C++ destroys members in the
  // reverse of their declaration, so they stand here in the reverse of the order in which they must go (`eng`, first
  // above, goes last):
  // RCCL communicator + events of the C++ halo loop (sf_halo_rccl.hip): only that file sees the RCCL headers
  OpaqueSlot halo;
  // the compute rdf commands, the cutoff grids and their device buffers (sf_nbr.hip): goes after the fixes ave/time, whose
  // samples read its arrays
  OpaqueSlot nbr;
  // the chunk/atom computes over c_ID and the per-chunk computes (sf_pchunk.hip): after the fixes ave/time, whose samples read
  // their arrays, and after the dumps, whose frames read the chunk IDs
  OpaqueSlot pchunks;
  // the per-atom computes and their device buffers (sf_compute_atom.hip): goes after the dumps, whose frames read them
  OpaqueSlot atom_computes;
  // the `compute pair/local` commands and the device scratch of their rows (sf_contacts.hip): after the dumps, likewise
  OpaqueSlot computes;
  // the chunk/atom computes, the fix ave/chunk commands, their device buffers and files (sf_chunk.hip): closes the files of
  // fix ave/chunk; after the dumps, like computes
  OpaqueSlot chunks;
  // the global computes, the fix ave/time commands, their device values, accumulators and files (sf_global.hip): closes the
  // files of fix ave/time
  OpaqueSlot globals;
  // the fix ave/histo commands, their device counters and files (sf_histo.hip): closes the files of fix ave/histo
  OpaqueSlot histos;
  // the `dump` commands and their writer thread (sf_dump.hip), which only that file sees: drains the writer, so that the
  // frames are in their files, before the computes they read go
  OpaqueSlot dumps;
  // thermo settings, destinations and the last line (sf_thermo.hip): closes the log and screen files
  OpaqueSlot thermo;
  // the `restart` schedule, the fix IDs of the walls and the wall rows of a restart file (sf_restart.hip)
  OpaqueSlot restart;
  // the device scratch of the image-count query and of the tags lammps_create_particle tells the displacement computes about
  // (sf_displace.hip)
  OpaqueSlot displace;
  // the regions, the dynamic groups, their programs and member counts on the device (sf_region.hip): goes first
  OpaqueSlot regions;
};

inline SfLammps* handle(void* p)
{
  if (!p) fail("null engine handle");
  return static_cast<SfLammps*>(p);
}

// the convention of the host-only *_parse.h / sf_compute_ref.h headers: an empty string, or the error text
inline void fail_if(const std::string& err)
{
  if (!err.empty()) fail("%s", err.c_str());
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
