// sf_gather_col.h -- the column descriptor of the whole-bed gathers and its loader: one value per element (an owned atom, or a
// row of a compute pair/local) from a component of a state record, a field-major buffer of doubles or ints, or a ke /
// erotate term.  k_global_gather (sf_global.hip: compute reduce, ke, erotate/sphere) and k_histo_bin (sf_histo.hip: fix
// ave/histo) take a by-value table of these and decode them with the one loader below.
#pragma once
#include <hip/hip_runtime.h>

#include "sf_atom_terms.h"

namespace sf {

enum GSrc { GS_XR, GS_VM, GS_OM, GS_FORCE, GS_TORQUE, GS_PTR, GS_INT, GS_ZERO, GS_ONE, GS_KE, GS_EROT };
enum GNeed { GN_XR = 1, GN_VM = 2, GN_OM = 4, GN_FORCE = 8, GN_TORQUE = 16, GN_MASK = 32 };

struct GCol {
  const void* p;   // GS_PTR: doubles indexed by element; GS_INT: ints
  int code;        // src | comp << 8 | op << 16 (comp: x y z w of a record); packed: the table lives in scalar registers
  int groupbit;    // 0: every element (rows)
  __host__ __device__ int src() const { return code & 255; }
  __host__ __device__ int comp() const { return (code >> 8) & 255; }
  __host__ __device__ int op() const { return code >> 16; }
  void set(int src, int comp, int op) { code = src | comp << 8 | op << 16; }
};
inline GCol make_col(const void* p, int src, int comp, int groupbit, int op)
{
  GCol c;
  c.p = p;
  c.groupbit = groupbit;
  c.set(src, comp, op);
  return c;
}
struct GRecords {
  const double4 *xr, *vm, *om, *force, *torque;
  const int* mask;
};

// the records a column reads (GNeed bits): a launch loads each record its table needs once per element
inline unsigned need_of(const GCol& c)
{
  unsigned need = c.groupbit ? GN_MASK : 0u;
  switch (c.src()) {
    case GS_XR: need |= GN_XR; break;
    case GS_VM:
    case GS_KE: need |= GN_VM; break;
    case GS_OM: need |= GN_OM; break;
    case GS_FORCE: need |= GN_FORCE; break;
    case GS_TORQUE: need |= GN_TORQUE; break;
    case GS_EROT: need |= GN_XR | GN_VM | GN_OM; break;
    default: break;
  }
  return need;
}

__device__ __forceinline__ double g_comp(const double4& a, int c) { return c == 0 ? a.x : (c == 1 ? a.y : (c == 2 ? a.z : a.w)); }

// the value of column c at element i; xr ... tq: the records of element i that the launch has loaded (need_of)
__device__ __forceinline__ double g_value(const GCol& c, long long i, const double4& xr, const double4& vm, const double4& om,
                                          const double4& f, const double4& tq)
{
  double v;
  switch (c.src()) {
    case GS_XR: v = g_comp(xr, c.comp()); break;
    case GS_VM: v = g_comp(vm, c.comp()); break;
    case GS_OM: v = g_comp(om, c.comp()); break;
    case GS_FORCE: v = g_comp(f, c.comp()); break;
    case GS_TORQUE: v = g_comp(tq, c.comp()); break;
    case GS_PTR: v = static_cast<const double*>(c.p)[i]; break;
    case GS_INT: v = (double)static_cast<const int*>(c.p)[i]; break;
    case GS_ONE: v = 1.0; break;
    case GS_KE: v = atom_ke_term(vm); break;
    case GS_EROT: v = atom_erotate_term(vm, om, xr.w); break;
    default: v = 0.0; break;
  }
  return v;
}

}  // namespace sf
