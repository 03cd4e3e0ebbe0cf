// sf_unmap.h -- the unwrapped coordinate ([3P] Domain::unmap for an orthogonal box): x + image * prd per component, the
// one definition behind xu yu zu of compute property/atom, compute displace/atom and compute com.
// The product and the sum are rounded separately -- floating-point contraction is off in these functions, whatever the
// file that includes them is compiled with -- so that NumPy's x + ix * L gives the same bits.  The image counts are the
// engine's (DemEngine::images_enable): three ints per TAG.
#pragma once
#include <hip/hip_runtime.h>

namespace sf {

// the table as an evaluation kernel sees it; rows: tags 0 .. rows - 1 have a row
struct ImageView {
  const int* image;
  int rows;
  double prd[3];   // box lengths, boxhi - boxlo as k_pbc_keys forms them
};

__device__ __forceinline__ double unmap1(double x, int image, double prd)
{
#pragma clang fp contract(off)
  const double shift = (double)image * prd;
  return x + shift;
}

// row `tag` of the table (zeros for a tag outside it)
__device__ __forceinline__ void image_of(const ImageView& V, int tag, int im[3])
{
  const bool ok = tag >= 0 && tag < V.rows;
  const int* p = V.image + 3 * (size_t)(ok ? tag : 0);
  im[0] = ok ? p[0] : 0;
  im[1] = ok ? p[1] : 0;
  im[2] = ok ? p[2] : 0;
}

__device__ __forceinline__ void unmap(const double4& x, const int im[3], const ImageView& V, double xu[3])
{
  xu[0] = unmap1(x.x, im[0], V.prd[0]);
  xu[1] = unmap1(x.y, im[1], V.prd[1]);
  xu[2] = unmap1(x.z, im[2], V.prd[2]);
}

// The correctly rounded square root, as NumPy's: the compiler's f64 sqrt is within one ulp, and from such a start one
// step with the exact residual -- r = x - s s by fma, s + r / (2 s) by fma -- rounds correctly (Markstein's theorem).
// x >= 0; tiny arguments are scaled by an even power of two so that the residual stays exact.
__device__ __forceinline__ double sqrt_rn(double x)
{
  if (!(x > 0.0)) return x;
  const bool tiny = x < 0x1p-900;
  const double xs = tiny ? x * 0x1p+200 : x;
  const double s = sqrt(xs);
  const double h = 0.5 / s;
  const double r = fma(-s, s, xs);
  const double g = fma(r, h, s);
  return tiny ? g * 0x1p-100 : g;
}

// sqrt((dx^2 + dy^2) + dz^2), every operation rounded on its own: the fourth column of compute displace/atom
__device__ __forceinline__ double length_rn(double dx, double dy, double dz)
{
#pragma clang fp contract(off)
  const double sx = dx * dx, sy = dy * dy, sz = dz * dz;
  const double sxy = sx + sy;
  return sqrt_rn(sxy + sz);
}

// a - b, rounded once (a difference that no product around it is fused into)
__device__ __forceinline__ double sub_rn(double a, double b)
{
#pragma clang fp contract(off)
  return a - b;
}

}  // namespace sf
