// sf_displace.hip -- the shared part of the unwrapped-coordinate keywords: xu yu zu ix iy iz of
// compute property/atom, compute displace/atom, compute com.
//   image_view       what a keyword needs of the engine: one rank, no fix rigid/nve, image counts kept from the start
//   RefTable         the reference positions of a displacement compute, by tag
//   k_ref_fill       x0[tag[i]] = unmap(x[i]), for every owned atom or for the marked rows only
//   k_ref_mark       marks the rows of a list of tags (the atoms lammps_create_particle has just made)
//   sf_lammps_get_image   the image counts of the owned atoms, gathered by tag into the engine's atom order
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/sedifoam_amd.h"
#include "sf_compute_atom.h"
#include "sf_displace.h"

namespace sf {
namespace {

// a row whose first word is this pattern waits for its reference (no unwrapped coordinate is a NaN)
__device__ __forceinline__ bool ref_marked(double v) { return v != v; }

__global__ __launch_bounds__(256) void k_ref_mark(const int* tags, int np, double* x0, int rows)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= np) return;
  const int t = tags[k];
  if (t >= 0 && t < rows) x0[3 * (size_t)t] = __longlong_as_double(0x7ff8000000000000ll);
}

__global__ __launch_bounds__(256) void k_ref_fill(const double4* xr, const int* tag, int n, ImageView V, int marked_only,
                                                  double* x0, int rows)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = tag[i];
  if (t < 0 || t >= rows) return;
  double* r = x0 + 3 * (size_t)t;
  if (marked_only && !ref_marked(r[0])) return;
  int im[3];
  double xu[3];
  image_of(V, t, im);
  unmap(xr[i], im, V, xu);
  r[0] = xu[0];
  r[1] = xu[1];
  r[2] = xu[2];
}

__global__ __launch_bounds__(256) void k_image_gather(const int* tag, int n, ImageView V, int* out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int im[3];
  image_of(V, tag[i], im);
  out[3 * (size_t)i] = im[0];
  out[3 * (size_t)i + 1] = im[1];
  out[3 * (size_t)i + 2] = im[2];
}

struct Staging {   // device scratch of this file, grown and kept
  std::vector<int> h;   // the tags of a lammps_create_particle call on their way to the device ...
  int* d = nullptr;     // ... and there
  size_t n = 0;
  int* img = nullptr;   // sf_lammps_get_image: [3 nlocal]
  size_t img_n = 0;
  ~Staging()
  {
    if (d) (void)hipFree(d);
    if (img) (void)hipFree(img);
  }
};

Staging& staging_of(SfLammps& L) { return L.displace.ensure<Staging>(); }

}  // namespace

ImageView image_view(SfLammps& L, const char* who)
{
  DemEngine& e = L.eng;
  refuse_decomposed(L, who);
  if (e.rigid_on())
    fail("%s: not while fix rigid/nve exists (the rigid integrator places the atoms of a body itself: their periodic images "
         "are not counted)", who);
  if (!e.images_enable())
    fail("%s: this engine has wrapped atoms around the periodic box without counting (no keyword had asked for image "
         "counts before the first run): give the compute before the first run", who);
  ImageView V;
  V.image = e.d_image();
  V.rows = e.image_rows();
  e.box_lengths(V.prd);
  return V;
}

RefTable::~RefTable()
{
  if (x0) (void)hipFree(x0);
}

void RefTable::fit(DemEngine& e)
{
  const size_t need = (size_t)e.max_tag() + 1;
  if (x0 && need <= rows) return;
  hipStream_t st = e.stream();
  const size_t nrows = need + need / 4 + 1024;
  double* p = nullptr;
  SF_HIP(hipMalloc(&p, sizeof(double) * 3 * nrows));
  SF_HIP(hipMemsetAsync(p, 0, sizeof(double) * 3 * nrows, st));
  if (x0) {
    SF_HIP(hipMemcpyAsync(p, x0, sizeof(double) * 3 * rows, hipMemcpyDeviceToDevice, st));
    SF_HIP(hipStreamSynchronize(st));   // (a launch queued on the stream may still read the old table)
    SF_HIP(hipFree(x0));
  }
  x0 = p;
  rows = nrows;
}

void ref_set_all(SfLammps& L, RefTable& R, const ImageView& V)
{
  DemEngine& e = L.eng;
  R.fit(e);
  const int n = e.nlocal();
  if (!n) return;
  k_ref_fill<<<div_up(n, 256), 256, 0, e.stream()>>>(e.d_xr(), e.d_tag(), n, V, 0, R.x0, (int)R.rows);
  SF_HIP(hipGetLastError());
}

void ref_set_tags(SfLammps& L, RefTable& R, const ImageView& V, const int* d_tags, int np)
{
  DemEngine& e = L.eng;
  R.fit(e);
  const int n = e.nlocal();
  if (!n || np <= 0) return;
  k_ref_mark<<<div_up(np, 256), 256, 0, e.stream()>>>(d_tags, np, R.x0, (int)R.rows);
  k_ref_fill<<<div_up(n, 256), 256, 0, e.stream()>>>(e.d_xr(), e.d_tag(), n, V, 1, R.x0, (int)R.rows);
  SF_HIP(hipGetLastError());
}

void displace_created(SfLammps& L, const double* tags, int np)
{
  if (np <= 0 || !tags || !L.eng.images_on()) return;   // (no table: no displacement compute)
  if (!atom_compute_tracks_created(L)) return;
  Staging& S = staging_of(L);
  hipStream_t st = L.eng.stream();
  if ((size_t)np > S.n) {
    if (S.d) {
      SF_HIP(hipStreamSynchronize(st));
      SF_HIP(hipFree(S.d));
      S.d = nullptr;
    }
    S.n = (size_t)np + 1024;
    SF_HIP(hipMalloc(&S.d, sizeof(int) * S.n));
  }
  SF_HIP(hipStreamSynchronize(st));   // (the copy of an earlier call may still read S.h; create_particles has waited anyway)
  S.h.resize(np);
  for (int k = 0; k < np; k++) S.h[k] = (int)tags[k];   // (library.cpp:437, as create_particles reads them)
  SF_HIP(hipMemcpyAsync(S.d, S.h.data(), sizeof(int) * (size_t)np, hipMemcpyHostToDevice, st));
  atom_compute_created(L, S.d, np);
}

}  // namespace sf

using sf::handle;

extern "C" {

int sf_lammps_get_image(void* ptr, int* out)
{
  SF_API_BEGIN
  sf::SfLammps& L = *handle(ptr);
  const int n = L.eng.nlocal();
  if (n > 0 && !out) sf::fail("sf_lammps_get_image: null argument");
  const sf::ImageView V = sf::image_view(L, "sf_lammps_get_image");
  if (n > 0) {
    hipStream_t st = L.eng.stream();
    sf::Staging& S = sf::staging_of(L);
    if (3 * (size_t)n > S.img_n) {
      if (S.img) {
        SF_HIP(hipStreamSynchronize(st));
        SF_HIP(hipFree(S.img));
        S.img = nullptr;
      }
      S.img_n = 3 * (size_t)n + 3 * (size_t)n / 4 + 4096;
      SF_HIP(hipMalloc(&S.img, sizeof(int) * S.img_n));
    }
    sf::k_image_gather<<<sf::div_up(n, 256), 256, 0, st>>>(L.eng.d_tag(), n, V, S.img);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(out, S.img, sizeof(int) * 3 * (size_t)n, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
  }
  SF_API_END(0)
}

}  // extern "C"
