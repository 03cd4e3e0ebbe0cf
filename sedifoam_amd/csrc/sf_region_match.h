// sf_region_match.h -- a region as the GPU sees it: a flat program of at most kRegionMaxPrims
// primitives, each with its side bit, and a postfix list of and / or / not steps; and region_match, the one predicate behind
// `group ID region`, `group ID dynamic ... region` and sf_lammps_region_match.  Plain data and plain arithmetic, compiled
// for the host (the stand-alone check of tests/c_abi) and for the device (sf_region.hip): every expression is rounded
// operation by operation -- floating-point contraction is off in these functions, whatever the file that includes them is
// compiled with -- so that NumPy gives the same bits, boundary points included.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include "sf_unmap.h"
#define SF_REGION_HD __host__ __device__
#else
#define SF_REGION_HD
#endif

namespace sf {

constexpr int kRegionMaxPrims = 16;   // primitives of one flattened region
constexpr int kRegionMaxSteps = 64;   // 16 pushes, 15 and/or, a not per union/intersect node (at most 15) and one to spare
constexpr double kRegionBig = 1.0e20;   // INF ([3P] LAMMPS' BIG)

enum RegionStyle { RS_BLOCK, RS_SPHERE, RS_CYLINDER, RS_PLANE, RS_UNION, RS_INTERSECT };
// a step of the program: 0 .. 15 pushes the match of that primitive; the others work on the top of the stack
enum RegionStep { RP_AND = 16, RP_OR = 17, RP_NOT = 18 };

// block: a = xlo xhi ylo yhi zlo zhi.  sphere: a = x y z r.  cylinder: axis 0 1 2, a = c1 c2 r lo hi.
// plane: a = px py pz n0 n1 n2 (the normal has length one)
struct RegionPrim {
  int style;
  int side_out;   // 1: the primitive matches where the point is NOT inside
  int axis;
  int pad;
  double a[6];
};

struct RegionProgram {
  int nprim;
  int nstep;
  int step[kRegionMaxSteps];   // (words: a wave reads them with scalar loads, which have no byte form on gfx950)
  RegionPrim prim[kRegionMaxPrims];
};

// the square root rounded correctly: the host's is; the device's is within one ulp and sqrt_rn corrects it
SF_REGION_HD inline double region_sqrt(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return sqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}

SF_REGION_HD inline bool region_inside(const RegionPrim& p, double x, double y, double z)
{
#if defined(__clang__)   // (g++ takes -ffp-contract=off on its command line)
#pragma clang fp contract(off)
#endif
  switch (p.style) {
    case RS_BLOCK:
      return x >= p.a[0] && x <= p.a[1] && y >= p.a[2] && y <= p.a[3] && z >= p.a[4] && z <= p.a[5];
    case RS_SPHERE: {
      const double dx = x - p.a[0], dy = y - p.a[1], dz = z - p.a[2];
      const double sx = dx * dx, sy = dy * dy, sz = dz * dz;
      const double sxy = sx + sy;
      return region_sqrt(sxy + sz) <= p.a[3];
    }
    case RS_CYLINDER: {
      // c1 c2 in LAMMPS' order: y z for x, x z for y, x y for z
      const double u = p.axis == 0 ? y : x, v = p.axis == 2 ? y : z, w = p.axis == 0 ? x : (p.axis == 1 ? y : z);
      const double d1 = u - p.a[0], d2 = v - p.a[1];
      const double s1 = d1 * d1, s2 = d2 * d2;
      return region_sqrt(s1 + s2) <= p.a[2] && w >= p.a[3] && w <= p.a[4];
    }
    default: {   // RS_PLANE
      const double t0 = (x - p.a[0]) * p.a[3], t1 = (y - p.a[1]) * p.a[4], t2 = (z - p.a[2]) * p.a[5];
      const double t01 = t0 + t1;
      return t01 + t2 >= 0.0;
    }
  }
}

// The match of one point.  The stack is a word of bits (bit 0 the top): the walk is the same for every point, so the lanes
// of a wave do not diverge in it, and a program is at most kRegionMaxPrims deep.
SF_REGION_HD inline bool region_match(const RegionProgram& P, double x, double y, double z)
{
  unsigned stk = 0u;
  for (int s = 0; s < P.nstep; s++) {
    const unsigned op = (unsigned)P.step[s];
    if (op < (unsigned)kRegionMaxPrims) {
      const RegionPrim& p = P.prim[op];
      const unsigned m = (region_inside(p, x, y, z) ? 1u : 0u) ^ (unsigned)(p.side_out & 1);
      stk = (stk << 1) | m;
    } else if (op == RP_NOT) {
      stk ^= 1u;
    } else {
      const unsigned t = stk & 1u;
      stk >>= 1;
      stk = op == RP_AND ? (stk & (~1u | t)) : (stk | t);
    }
  }
  return (stk & 1u) != 0u;
}

}  // namespace sf
