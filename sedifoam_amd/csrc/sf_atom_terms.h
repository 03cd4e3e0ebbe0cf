// sf_atom_terms.h -- the per-atom energy terms that compute ke/atom and erotate/sphere/atom (sf_compute_atom.hip) store and
// that compute ke and compute erotate/sphere (sf_global.hip) sum: one definition, so that the global value is the sum of
// the per-atom column up to the order of the summation.
#pragma once
#include <hip/hip_runtime.h>

namespace sf {

// vm = (vx, vy, vz, mass): 1/2 m v^2
__device__ __forceinline__ double atom_ke_term(const double4& v) { return 0.5 * v.w * (v.x * v.x + v.y * v.y + v.z * v.z); }

// om = (wx, wy, wz, .), r the radius: 1/2 (0.4 m r^2) omega^2  ([3P] ComputeERotateSphereAtom, INERTIA = 0.4)
__device__ __forceinline__ double atom_erotate_term(const double4& v, const double4& w, double r)
{
  return 0.5 * (0.4 * v.w * r * r) * (w.x * w.x + w.y * w.y + w.z * w.z);
}

}  // namespace sf
