// sf_feed.h -- the cloud's particle add / delete schedules (cloudProperties addParticle, deleteParticle, deleteBeforeAdd):
//   pointInRegion          softParticleCloud.C:1354-1417   point_in_region (host and device)
//   findAddParticleCells   softParticleCloud.C:1271-1352   feed_add_cells (host, once)
//   Random(size())         softParticleCloud.C:1183        Lcg48: the 48-bit generator of drand48 with skip-ahead
// and what sf_feed.hip gives the cloud: the mark and the create launches (DemEngine::feed_*, declared in sf_dem.h).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "sf_common.h"

namespace sf {

struct SfLammps;

constexpr double kRootVSmall = 1.0e-150;  // OpenFOAM ROOTVSMALL (double precision)

// softParticleCloud::pointInRegion  softParticleCloud.C:1354-1417 (option 1: box, faces included; option 2: between the
// cylinders r1 -- shifted by the eccentricity -- and r2 around the axis (x1,y1,z1)-(x2,y2,z2); as there, the inner
// distance uses the projection of the UNshifted point; any other option: nowhere)
__host__ __device__ __forceinline__ bool point_in_region(int option, const double* b, const double* ecc, double px,
                                                         double py, double pz)
{
  const double x1 = b[0], x2 = b[1], y1 = b[2], y2 = b[3], z1 = b[4], z2 = b[5], r1 = b[6], r2 = b[7];
  if (option == 1)
    return (px - x1) * (px - x2) < kRootVSmall && (py - y1) * (py - y2) < kRootVSmall && (pz - z1) * (pz - z2) < kRootVSmall;
  if (option == 2) {
    const double a[3] = {x2 - x1, y2 - y1, z2 - z1}, q[3] = {px - x1, py - y1, pz - z1};
    const double h = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double dot = a[0] * q[0] + a[1] * q[1] + a[2] * q[2];
    if (dot < 0.0 || dot > pow(h, 2)) return false;
    const double qe[3] = {q[0] - ecc[0], q[1] - ecc[1], q[2] - ecc[2]};
    const double dsq = (q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) - dot * dot / pow(h, 2);
    const double dsqE = (qe[0] * qe[0] + qe[1] * qe[1] + qe[2] * qe[2]) - dot * dot / pow(h, 2);
    return dsqE > r1 * r1 && dsq < r2 * r2;
  }
  return false;
}

// The generator of srand48 / drand48: X' = (a X + c) mod 2^48, X0 = (seed << 16) | 0x330E, u = X / 2^48.  step^n is an
// affine map again; skip(n) composes it by square-and-multiply, so draw k costs log2 k multiplications.  As srand48 does,
// the constructor takes the low 32 bits of the seed.
struct Lcg48 {
  static constexpr uint64_t kMask = (1ull << 48) - 1ull, kA = 0x5DEECE66Dull, kC = 0xBull;
  uint64_t x;
  __host__ __device__ explicit Lcg48(uint64_t seed) : x(((seed & 0xffffffffull) << 16) | 0x330Eull) {}
  __host__ __device__ void skip(uint64_t n)
  {
    uint64_t ra = 1, rc = 0, ba = kA, bc = kC;
    for (; n; n >>= 1) {
      if (n & 1) {
        ra = (ba * ra) & kMask;
        rc = (ba * rc + bc) & kMask;
      }
      bc = (ba * bc + bc) & kMask;
      ba = (ba * ba) & kMask;
    }
    x = (ra * x + rc) & kMask;
  }
  __host__ __device__ double next()   // drand48()
  {
    x = (kA * x + kC) & kMask;
    return (double)x * (1.0 / 281474976710656.0);   // (exact: X < 2^48, the factor a power of two)
  }
};

// what the mark kernel is given by value
struct FeedMark {
  int option;        // region kind of every box (addParticle)
  int clear;         // test clearInitialBox: an add is due, with deleteBeforeAdd and deleteParticle > 0
  int del;           // test deleteParticleBox
  int flag_cleared;  // leave_ takes the cleared grains (the compaction before an add) instead of the deleted ones
  int tag_limit;     // grains with a higher tag are not looked at (the grains an add has just made)
  double clearBox[9], deleteBox[9], ecc[3];
};
struct FeedCounts {
  int cleared, deleted, maxtag;   // maxtag: the largest tag among the grains not cleared (0: none)
};

// what the create kernel is given by value (the row pointers come from the engine)
struct FeedCreate {
  int np, first_tag, type, mask;
  double radius, mass, vel[3], perturb;
  uint64_t seed;
  const double* centres;   // [np][3] device: the add cells' centres
};

// findAddParticleCells on a tensor-product mesh: centres[3 ncells] in OpenFOAM label order; returns the selected labels
inline std::vector<int> feed_add_cells(int option, const double* box, const double* ecc, const std::vector<double>& centres,
                                       int reduceNumberFactor)
{
  const int ncells = (int)(centres.size() / 3);
  auto inside = [&](int c) { return point_in_region(option, box, ecc, centres[3 * c], centres[3 * c + 1], centres[3 * c + 2]); };
  int nCell = 0;
  for (int c = 0; c < ncells; c++) nCell += inside(c) ? 1 : 0;
  const int coarse = reduceNumberFactor;
  const int nLine = (int)std::pow((double)nCell, 0.5);
  std::vector<int> out;
  int i = 0;
  for (int c = 0; c < ncells; c++) {
    if (!inside(c)) continue;
    const int nRow = i % coarse, nColumn = i / nLine;   // (nCell >= 1 here, so nLine >= 1)
    if (nRow % coarse == 0 && nColumn % coarse == 0) out.push_back(c);
    i++;
  }
  return out;
}

// what sf_lammps_create_particle / sf_lammps_delete_particle do around the engine call, for them and for the cloud's feed
// (sf_lammps_api.hip): the rigid-body refusal, the per-atom computes, the image counts / the displacement references
void particles_change_begin(SfLammps& L, const char* who, bool creating);
void particles_created_end(SfLammps& L, const double* tags, int np);
void particles_deleted_end(SfLammps& L);

}  // namespace sf
