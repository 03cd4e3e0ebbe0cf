// sf_rigid.h -- fix rigid/nve ([3P] LAMMPS 1Feb14 FixRigidNVE) for bodies of spheres on one GPU (sf_rigid.hip).
//
// Per atom (DemEngine::rigid_rows_, [kRigidRows][cap] doubles, permuted by every re-sort like the client rows):
//   row 0      body index (-1: none), bodies numbered by the smallest tag they hold
//   rows 1-3   displace: the atom's position relative to the centre of mass in the body's principal frame
//   row 4      mbody: the mass the PAIR law sees -- the body's total mass, or the atom's own when it is in no body
//              (pair_gran_hertzFix_history.cpp:72-86, 182-185)
//   row 5      molecule ID (fix property/atom mol, read_data ... fix ID NULL Molecules, sf_lammps_set_molecule)
// Per body: a [kBodyFields][nbody] array of doubles on the device (field-major: lane b reads consecutive addresses).
//
// One sub-step with the fix: k_substep<RIGID> (forces only, into force / torque) -> body reduction (slot order, no
// floating-point atomics) -> k_rigid_integrate (final half of step k + initial half of step k + 1, one lane per body)
// -> k_rigid_writeback (one lane per atom: body atoms from their body, free nve/sphere atoms integrated, the rest
// copied; next ping-pong records; skin / 2 test).  Every kernel leaves at once when the trigger word says the list
// went stale in an earlier sub-step of the queue.
#pragma once
#include <vector>

#include "sf_dem.h"

namespace sf {

constexpr int kRigidRows = 6;
enum RigidRow { RR_BODY = 0, RR_DISP = 1, RR_MBODY = 4, RR_MOL = 5 };

enum BodyField {
  BF_XCM = 0,
  BF_VCM = 3,
  BF_FCM = 6,
  BF_TORQUE = 9,
  BF_ANGMOM = 12,
  BF_OMEGA = 15,
  BF_CONJQM = 18,
  BF_QUAT = 22,
  BF_INERTIA = 26,
  BF_MASS = 29,
  BF_EX = 30,   // principal axes in the space frame: ex, ey, ez (3 each)
  kBodyFields = 39
};

constexpr int kRigidSmall = 64;    // bodies of up to this many atoms: one lane sums the body's slots in order
constexpr int kRigidChunk = 256;   // larger bodies: partial sums over chunks of this many slots, then one block per body

struct RigidFix {
  int bodystyle = 0;               // 0 single, 1 group, 2 molecule
  int groupbit = 1;
  std::vector<int> groupbits;      // `group N g1 ... gN`
  bool dirty = true;               // the bodies must be derived from the atoms again
  int nbody = 0;
  long long nin = 0;               // atoms that belong to a body
  std::vector<int> natoms;         // per body
  std::vector<int> off;            // CSR offsets of the body -> atom map (constant while the fix lives)
  int nsmall = 0, nlarge = 0, nchunks = 0;
  // device
  double* bs = nullptr;            // [kBodyFields][nbody]
  int* d_off = nullptr;            // [nbody + 1]
  int* d_small = nullptr;          // ids of the small bodies
  int* d_large = nullptr;          // ids of the large bodies, then their first chunk and chunk count (3 rows)
  int* d_chunk = nullptr;          // [3][nchunks]: body, first slot, end slot
  double* d_part = nullptr;        // [nchunks][6] partial sums
  unsigned* keys[2] = {nullptr, nullptr};
  int* vals[2] = {nullptr, nullptr};   // vals[1]: the map (atom indices, body by body, index order inside a body)
  size_t map_cap = 0;
  void* sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  bool map_valid = false;
  bool force_stale = true;         // fcm / torque do not hold the sums of the last force evaluation (new bodies)
  void release();
};

// the RIGID instantiations of k_substep (one lane per atom, v / omega of every neighbour requested, nothing non-temporal)
void launch_substep_rigid(int style, bool cohe, bool lub, dim3 grid, int block, hipStream_t s, const DemPtrs& P,
                          const StepParams& S);

}  // namespace sf
