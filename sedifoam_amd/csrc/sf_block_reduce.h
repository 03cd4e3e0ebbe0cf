// sf_block_reduce.h -- the block step of the whole-bed reductions (thermo's k_thermo_reduce / k_thermo_virial, the global
// computes of sf_global.hip): NV values per thread -> one row of NV values per block.  A shuffle tree inside each wave64,
// then the waves' partials through LDS, combined in wave order by the first NV threads.  No atomics: the order of every
// combination is fixed, so the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace sf {

// comb(c, a, b): the combination of component c (a sum, a maximum, a minimum); it is called with a compile-time c in the
// wave tree and with c = threadIdx.x in the last step.  Components c >= nuse (uniform over the block) are left alone and
// not stored.  Every thread of the block calls this, once per kernel (one static LDS buffer) -- or again with the same
// BLOCK and NV only behind a __syncthreads() that every thread passes after the earlier call (k_global_unwrapped).
template <int BLOCK, int NV, class Combine>
__device__ __forceinline__ void block_reduce_store(double (&v)[NV], double* out, int nuse, Combine comb)
{
  __shared__ double ws[BLOCK / 64][NV];
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int c = 0; c < NV; c++)
      if (c < nuse) {
        const double o = __shfl_down(v[c], off, 64);
        v[c] = comb(c, v[c], o);
      }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int c = 0; c < NV; c++) ws[w][c] = v[c];
  __syncthreads();
  if ((int)threadIdx.x < NV && (int)threadIdx.x < nuse) {
    const int c = threadIdx.x;
    double t = ws[0][c];
    for (int k = 1; k < BLOCK / 64; k++) t = comb(c, t, ws[k][c]);
    out[c] = t;
  }
}

}  // namespace sf
