// sf_rigid.hip -- fix rigid/nve: bodies of spheres integrated on the GPU (see sf_rigid.h for the layout and the kernel
// sequence, DESIGN.md section 11 for the rules).  [3P] LAMMPS 1Feb14 FixRigidNVE is the target: symplectic NO_SQUISH
// rotation (Miller et al., J Chem Phys 116, 8649 (2002)) of a quaternion and its conjugate momentum.
#include "sf_rigid.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <map>

#include "sf_dem_dispatch.h"
#include "sf_dem_kernels.h"

namespace sf {

// ------------------------------------------------------------------------------------------------
// the force evaluation: k_substep with the body-mass branch of the pair law, storing force / torque only
// ------------------------------------------------------------------------------------------------
void launch_substep_rigid(int style, bool cohe, bool lub, dim3 grid, int block, hipStream_t s, const DemPtrs& P,
                          const StepParams& S)
{
  pair_dispatch(style, cohe, lub, [&](auto st, auto c, auto l) {
    k_substep<st, c, l, 1, false, 0, false, true><<<grid, block, 0, s>>>(P, S);
  });
}

// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------
namespace {

struct RigidView {
  double* bs;            // [kBodyFields][nbody]
  int nbody;
  const double* rows;    // [kRigidRows][cap]
  size_t cap;
  const int* map;        // atom indices, body by body
  const int* off;        // [nbody + 1]
  int* flags;
};

__device__ __forceinline__ bool stale(const int* flags, int kstep)
{
  return __atomic_load_n(&flags[F_TRIGGER], __ATOMIC_RELAXED) < kstep;
}

__device__ __forceinline__ double bget(const RigidView& V, int f, int b) { return V.bs[(size_t)f * V.nbody + b]; }
__device__ __forceinline__ void bput(const RigidView& V, int f, int b, double v) { V.bs[(size_t)f * V.nbody + b] = v; }
__device__ __forceinline__ Vec3 bget3(const RigidView& V, int f, int b)
{
  return {bget(V, f, b), bget(V, f + 1, b), bget(V, f + 2, b)};
}
__device__ __forceinline__ void bput3(const RigidView& V, int f, int b, Vec3 v)
{
  bput(V, f, b, v.x);
  bput(V, f + 1, b, v.y);
  bput(V, f + 2, b, v.z);
}
__device__ __forceinline__ Vec3 cross(Vec3 a, Vec3 b)
{
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// space-frame vector of body-frame components d: ex d0 + ey d1 + ez d2
__device__ __forceinline__ Vec3 to_space(Vec3 ex, Vec3 ey, Vec3 ez, Vec3 d)
{
  return {ex.x * d.x + ey.x * d.y + ez.x * d.z, ex.y * d.x + ey.y * d.y + ez.y * d.z, ex.z * d.x + ey.z * d.y + ez.z * d.z};
}

__global__ __launch_bounds__(256) void k_rigid_keys(const double* body_row, int n, int nbody, unsigned* keys, int* vals)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b = (int)body_row[i];
  keys[i] = b < 0 ? (unsigned)nbody : (unsigned)b;   // atoms of no body sort behind every body
  vals[i] = i;
}

// what one atom adds to its body's force and torque: f, and (x_i - xcm) x f + t_i with x_i - xcm = R displace
struct Sum6 {
  double v[6];
};
__device__ __forceinline__ Sum6 atom_term(const RigidView& V, const double4* force, const double4* torque, int i, Vec3 ex,
                                          Vec3 ey, Vec3 ez)
{
  const double4 f = force[i], t = torque[i];
  const Vec3 d = {V.rows[(size_t)RR_DISP * V.cap + i], V.rows[(size_t)(RR_DISP + 1) * V.cap + i],
                  V.rows[(size_t)(RR_DISP + 2) * V.cap + i]};
  const Vec3 r = to_space(ex, ey, ez, d);
  const Vec3 c = cross(r, Vec3{f.x, f.y, f.z});
  return {{f.x, f.y, f.z, c.x + t.x, c.y + t.y, c.z + t.z}};
}

// bodies of up to kRigidSmall atoms: one lane walks the body's slots in order
__global__ __launch_bounds__(256) void k_rigid_reduce_small(RigidView V, const int* ids, int nsmall, const double4* force,
                                                            const double4* torque, int kstep)
{
  if (stale(V.flags, kstep)) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nsmall) return;
  const int b = ids[k];
  const Vec3 ex = bget3(V, BF_EX, b), ey = bget3(V, BF_EX + 3, b), ez = bget3(V, BF_EX + 6, b);
  Sum6 s = {{0, 0, 0, 0, 0, 0}};
  for (int q = V.off[b]; q < V.off[b + 1]; q++) {
    const Sum6 a = atom_term(V, force, torque, V.map[q], ex, ey, ez);
    for (int c = 0; c < 6; c++) s.v[c] += a.v[c];
  }
  bput3(V, BF_FCM, b, {s.v[0], s.v[1], s.v[2]});
  bput3(V, BF_TORQUE, b, {s.v[3], s.v[4], s.v[5]});
}

// fixed-shape tree over the 256 values of a block: shuffles inside a wave, then the four wave sums in order
__device__ __forceinline__ Sum6 block_tree_256(Sum6 s)
{
  __shared__ double ws[4][6];
  for (int c = 0; c < 6; c++)
    for (int o = 32; o > 0; o >>= 1) s.v[c] += __shfl_down(s.v[c], o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0)
    for (int c = 0; c < 6; c++) ws[w][c] = s.v[c];
  __syncthreads();
  Sum6 t;
  for (int c = 0; c < 6; c++) t.v[c] = (ws[0][c] + ws[1][c]) + (ws[2][c] + ws[3][c]);
  return t;   // (every thread holds the total)
}

// larger bodies, pass 1: one block per chunk of kRigidChunk slots of ONE body
__global__ __launch_bounds__(kRigidChunk) void k_rigid_partials(RigidView V, const int* chunk, int nchunks,
                                                                const double4* force, const double4* torque, double* part,
                                                                int kstep)
{
  if (stale(V.flags, kstep)) return;
  const int c = blockIdx.x;
  const int b = chunk[c], q = chunk[nchunks + c] + (int)threadIdx.x, end = chunk[2 * nchunks + c];
  Sum6 s = {{0, 0, 0, 0, 0, 0}};
  if (q < end) {
    const Vec3 ex = bget3(V, BF_EX, b), ey = bget3(V, BF_EX + 3, b), ez = bget3(V, BF_EX + 6, b);
    s = atom_term(V, force, torque, V.map[q], ex, ey, ez);
  }
  s = block_tree_256(s);
  if (threadIdx.x == 0)
    for (int k = 0; k < 6; k++) part[(size_t)c * 6 + k] = s.v[k];
}

// pass 2: one block per body over its chunk partials (thread t takes partials t, t + 256, ... in order)
__global__ __launch_bounds__(256) void k_rigid_reduce_large(RigidView V, const int* large, int nlarge, const double* part,
                                                            int kstep)
{
  if (stale(V.flags, kstep)) return;
  const int b = large[blockIdx.x], c0 = large[nlarge + blockIdx.x], nc = large[2 * nlarge + blockIdx.x];
  Sum6 s = {{0, 0, 0, 0, 0, 0}};
  for (int c = (int)threadIdx.x; c < nc; c += 256)
    for (int k = 0; k < 6; k++) s.v[k] += part[(size_t)(c0 + c) * 6 + k];
  s = block_tree_256(s);
  if (threadIdx.x == 0) {
    bput3(V, BF_FCM, b, {s.v[0], s.v[1], s.v[2]});
    bput3(V, BF_TORQUE, b, {s.v[3], s.v[4], s.v[5]});
  }
}

struct Quat {
  double w, x, y, z;
};
// q (x) (0, b)
__device__ __forceinline__ Quat quatvec(Quat a, Vec3 b)
{
  return {-a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.y * b.z - a.z * b.y, a.w * b.y + a.z * b.x - a.x * b.z,
          a.w * b.z + a.x * b.y - a.y * b.x};
}
// vector part of q^-1 (x) b
__device__ __forceinline__ Vec3 invquatvec(Quat a, Quat b)
{
  return {-a.x * b.w + a.w * b.x + a.z * b.y - a.y * b.z, -a.y * b.w - a.z * b.x + a.w * b.y + a.x * b.z,
          -a.z * b.w + a.y * b.x - a.x * b.y + a.w * b.z};
}
__device__ __forceinline__ void axes_of(Quat q, Vec3& ex, Vec3& ey, Vec3& ez)
{
  ex = {q.w * q.w + q.x * q.x - q.y * q.y - q.z * q.z, 2.0 * (q.x * q.y + q.w * q.z), 2.0 * (q.x * q.z - q.w * q.y)};
  ey = {2.0 * (q.x * q.y - q.w * q.z), q.w * q.w - q.x * q.x + q.y * q.y - q.z * q.z, 2.0 * (q.y * q.z + q.w * q.x)};
  ez = {2.0 * (q.x * q.z + q.w * q.y), 2.0 * (q.y * q.z - q.w * q.x), q.w * q.w - q.x * q.x - q.y * q.y + q.z * q.z};
}
// one factor of the NO_SQUISH splitting: rotation about principal axis k (1, 2, 3) for a time dt
__device__ __forceinline__ void no_squish_rotate(int k, Quat& p, Quat& q, const double (&I)[3], double dt)
{
  Quat kq, kp;
  if (k == 1) {
    kq = {-q.x, q.w, q.z, -q.y};
    kp = {-p.x, p.w, p.z, -p.y};
  } else if (k == 2) {
    kq = {-q.y, -q.z, q.w, q.x};
    kp = {-p.y, -p.z, p.w, p.x};
  } else {
    kq = {-q.z, q.y, -q.x, q.w};
    kp = {-p.z, p.y, -p.x, p.w};
  }
  double phi = p.w * kq.w + p.x * kq.x + p.y * kq.y + p.z * kq.z;
  phi = I[k - 1] == 0.0 ? 0.0 : phi / (4.0 * I[k - 1]);
  const double c = cos(dt * phi), s = sin(dt * phi);
  p = {c * p.w + s * kp.w, c * p.x + s * kp.x, c * p.y + s * kp.y, c * p.z + s * kp.z};
  q = {c * q.w + s * kq.w, c * q.x + s * kq.x, c * q.y + s * kq.y, c * q.z + s * kq.z};
}

// one lane per body: final half of a step (do_final), initial half of the next one (do_initial)
__global__ __launch_bounds__(64) void k_rigid_integrate(RigidView V, double dt, int do_final, int do_initial, int kstep,
                                                        double3 lo, double3 prd, int3 per)
{
  if (stale(V.flags, kstep)) return;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= V.nbody) return;
  const double dtf = 0.5 * dt;
  const double M = bget(V, BF_MASS, b);
  const double I[3] = {bget(V, BF_INERTIA, b), bget(V, BF_INERTIA + 1, b), bget(V, BF_INERTIA + 2, b)};
  Vec3 xcm = bget3(V, BF_XCM, b), vcm = bget3(V, BF_VCM, b);
  const Vec3 fcm = bget3(V, BF_FCM, b), tq = bget3(V, BF_TORQUE, b);
  Quat q = {bget(V, BF_QUAT, b), bget(V, BF_QUAT + 1, b), bget(V, BF_QUAT + 2, b), bget(V, BF_QUAT + 3, b)};
  Quat p = {bget(V, BF_CONJQM, b), bget(V, BF_CONJQM + 1, b), bget(V, BF_CONJQM + 2, b), bget(V, BF_CONJQM + 3, b)};
  Vec3 ex = bget3(V, BF_EX, b), ey = bget3(V, BF_EX + 3, b), ez = bget3(V, BF_EX + 6, b);
  const double dtfm = dtf / M;
  // the half kick (the same lines in both halves): vcm += dtf fcm / M, conjqm += dtf 2 q (x) (0, R^T torque)
  auto kick = [&]() {
    vcm = vcm + dtfm * fcm;
    const Vec3 tb = {dot(ex, tq), dot(ey, tq), dot(ez, tq)};
    const Quat fq = quatvec(q, tb);
    p = {p.w + dtf * 2.0 * fq.w, p.x + dtf * 2.0 * fq.x, p.y + dtf * 2.0 * fq.y, p.z + dtf * 2.0 * fq.z};
  };
  if (do_final) kick();
  if (do_initial) {
    kick();
    xcm = xcm + dt * vcm;
    const double dtq = 0.5 * dt;
    no_squish_rotate(3, p, q, I, dtq);
    no_squish_rotate(2, p, q, I, dtq);
    no_squish_rotate(1, p, q, I, dt);
    no_squish_rotate(2, p, q, I, dtq);
    no_squish_rotate(3, p, q, I, dtq);
    const double n = 1.0 / sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    q = {q.w * n, q.x * n, q.y * n, q.z * n};
    axes_of(q, ex, ey, ez);
    // the centre of mass stays in the box on periodic axes (the atoms are wrapped one by one: any image serves)
    if (per.x) xcm.x += xcm.x < lo.x ? prd.x : (xcm.x >= lo.x + prd.x ? -prd.x : 0.0);
    if (per.y) xcm.y += xcm.y < lo.y ? prd.y : (xcm.y >= lo.y + prd.y ? -prd.y : 0.0);
    if (per.z) xcm.z += xcm.z < lo.z ? prd.z : (xcm.z >= lo.z + prd.z ? -prd.z : 0.0);
  }
  // angmom = R (1/2 q^-1 (x) conjqm), omega = R (angmom_body / I)
  const Vec3 mb = invquatvec(q, p);
  const Vec3 lb = {0.5 * mb.x, 0.5 * mb.y, 0.5 * mb.z};
  const Vec3 L = to_space(ex, ey, ez, lb);
  const Vec3 wb = {I[0] == 0.0 ? 0.0 : dot(L, ex) / I[0], I[1] == 0.0 ? 0.0 : dot(L, ey) / I[1],
                   I[2] == 0.0 ? 0.0 : dot(L, ez) / I[2]};
  const Vec3 om = to_space(ex, ey, ez, wb);
  bput3(V, BF_XCM, b, xcm);
  bput3(V, BF_VCM, b, vcm);
  bput3(V, BF_ANGMOM, b, L);
  bput3(V, BF_OMEGA, b, om);
  bput(V, BF_QUAT, b, q.w); bput(V, BF_QUAT + 1, b, q.x); bput(V, BF_QUAT + 2, b, q.y); bput(V, BF_QUAT + 3, b, q.z);
  bput(V, BF_CONJQM, b, p.w); bput(V, BF_CONJQM + 1, b, p.x); bput(V, BF_CONJQM + 2, b, p.y); bput(V, BF_CONJQM + 3, b, p.z);
  bput3(V, BF_EX, b, ex);
  bput3(V, BF_EX + 3, b, ey);
  bput3(V, BF_EX + 6, b, ez);
}

struct WritebackArgs {
  const double4 *xi, *vi, *wi;
  double4 *xo, *vo, *wo;
  const double4 *force, *torque;
  const double* xhold;
  const int* mask;     // (nullptr: every fix is on `all`)
  int nlocal, have_nve, nve_bit;
  int do_final, do_initial, kstep;
  double dt, trigger_sq;
  double lo[3], prd[3];
  int per[3];
};

// one lane per atom: an atom of a body is placed by its body (x only when the bodies moved), a free atom of the
// fix nve/sphere group takes the same half kicks k_substep gives it, everything else is copied
__global__ __launch_bounds__(256) void k_rigid_writeback(RigidView V, WritebackArgs A)
{
  if (stale(V.flags, A.kstep)) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.nlocal) return;
  double4 x = A.xi[i], v = A.vi[i], w = A.wi[i];
  const int b = (int)V.rows[(size_t)RR_BODY * V.cap + i];
  bool moved = false;
  if (b >= 0) {
    const Vec3 ex = bget3(V, BF_EX, b), ey = bget3(V, BF_EX + 3, b), ez = bget3(V, BF_EX + 6, b);
    const Vec3 d = {V.rows[(size_t)RR_DISP * V.cap + i], V.rows[(size_t)(RR_DISP + 1) * V.cap + i],
                    V.rows[(size_t)(RR_DISP + 2) * V.cap + i]};
    const Vec3 r = to_space(ex, ey, ez, d);
    const Vec3 vcm = bget3(V, BF_VCM, b), om = bget3(V, BF_OMEGA, b);
    if (A.do_initial) {
      const Vec3 xcm = bget3(V, BF_XCM, b);
      double xn[3] = {xcm.x + r.x, xcm.y + r.y, xcm.z + r.z};
      for (int k = 0; k < 3; k++)
        if (A.per[k]) xn[k] += xn[k] < A.lo[k] ? A.prd[k] : (xn[k] >= A.lo[k] + A.prd[k] ? -A.prd[k] : 0.0);
      x.x = xn[0];
      x.y = xn[1];
      x.z = xn[2];
      moved = true;
    }
    const Vec3 c = cross(om, r);
    v.x = c.x + vcm.x;
    v.y = c.y + vcm.y;
    v.z = c.z + vcm.z;
    w.x = om.x;
    w.y = om.y;
    w.z = om.z;
  } else if (A.have_nve && (!A.mask || (A.mask[i] & A.nve_bit)) && (A.do_final || A.do_initial)) {
    // [3P] FixNVESphere, dtf = dt / 2, INERTIA = 0.4 (the lines of substep_particle)
    const double4 f = A.force[i], t = A.torque[i];
    const double dtf = 0.5 * A.dt;
    const double dtfm = dtf / v.w;
    const double dtirot = (dtf / 0.4) / (x.w * x.w * v.w);
    if (A.do_final) {
      v.x += dtfm * f.x; v.y += dtfm * f.y; v.z += dtfm * f.z;
      w.x += dtirot * t.x; w.y += dtirot * t.y; w.z += dtirot * t.z;
    }
    if (A.do_initial) {
      v.x += dtfm * f.x; v.y += dtfm * f.y; v.z += dtfm * f.z;
      x.x += A.dt * v.x; x.y += A.dt * v.y; x.z += A.dt * v.z;
      w.x += dtirot * t.x; w.y += dtirot * t.y; w.z += dtirot * t.z;
      moved = true;
    }
  }
  A.xo[i] = x;
  A.vo[i] = v;
  A.wo[i] = w;
  if (moved) {
    const double dx = x.x - A.xhold[i], dy = x.y - A.xhold[V.cap + i], dz = x.z - A.xhold[2 * V.cap + i];
    // (an atom wrapped across a periodic face has moved a box length: the list is rebuilt before it is used again)
    if (dx * dx + dy * dy + dz * dz > A.trigger_sq) atomicMin(&V.flags[F_TRIGGER], A.kstep);
  }
}

// ------------------------------------------------------------------------------------------------
// host side: the bodies from the atoms
// ------------------------------------------------------------------------------------------------
// cyclic Jacobi on a symmetric 3 x 3 matrix: a -> diagonal (the moments), the columns of v = the axes
void jacobi3(double a[3][3], double d[3], double v[3][3])
{
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; sweep++) {
    const double offd = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    const double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
    if (offd == 0.0 || offd <= 1e-300 + 1e-32 * diag) break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; k++) {   // columns p, q of a
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; k++) {   // rows p, q of a
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; k++) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int k = 0; k < 3; k++) d[k] = a[k][k];
}

// quaternion of the right-handed axis triple ex, ey, ez ([3P] MathExtra::exyz_to_q)
void quat_of_axes(const double ex[3], const double ey[3], const double ez[3], double q[4])
{
  const double q0sq = 0.25 * (ex[0] + ey[1] + ez[2] + 1.0);
  const double q1sq = q0sq - 0.5 * (ey[1] + ez[2]);
  const double q2sq = q0sq - 0.5 * (ex[0] + ez[2]);
  const double q3sq = q0sq - 0.5 * (ex[0] + ey[1]);
  q[0] = q[1] = q[2] = q[3] = 0.0;
  if (q0sq >= 0.25) {
    q[0] = sqrt(q0sq);
    q[1] = (ey[2] - ez[1]) / (4.0 * q[0]);
    q[2] = (ez[0] - ex[2]) / (4.0 * q[0]);
    q[3] = (ex[1] - ey[0]) / (4.0 * q[0]);
  } else if (q1sq >= 0.25) {
    q[1] = sqrt(q1sq);
    q[0] = (ey[2] - ez[1]) / (4.0 * q[1]);
    q[2] = (ey[0] + ex[1]) / (4.0 * q[1]);
    q[3] = (ex[2] + ez[0]) / (4.0 * q[1]);
  } else if (q2sq >= 0.25) {
    q[2] = sqrt(q2sq);
    q[0] = (ez[0] - ex[2]) / (4.0 * q[2]);
    q[1] = (ey[0] + ex[1]) / (4.0 * q[2]);
    q[3] = (ez[1] + ey[2]) / (4.0 * q[2]);
  } else {
    q[3] = sqrt(q3sq > 0.0 ? q3sq : 0.0);
    q[0] = (ex[1] - ey[0]) / (4.0 * q[3]);
    q[1] = (ez[0] + ex[2]) / (4.0 * q[3]);
    q[2] = (ez[1] + ey[2]) / (4.0 * q[3]);
  }
  const double n = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) q[k] *= n;
}

template <class T>
void dev_free(T*& p)
{
  if (p) (void)hipFree(p);
  p = nullptr;
}
template <class T>
void dev_upload(T*& p, const std::vector<T>& h, hipStream_t s)
{
  dev_free(p);
  SF_HIP(hipMalloc(&p, sizeof(T) * std::max<size_t>(h.size(), 1)));
  if (!h.empty()) SF_HIP(hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, s));
}

}  // namespace

void RigidFix::release()
{
  dev_free(bs);
  dev_free(d_off);
  dev_free(d_small);
  dev_free(d_large);
  dev_free(d_chunk);
  dev_free(d_part);
  dev_free(keys[0]);
  dev_free(keys[1]);
  dev_free(vals[0]);
  dev_free(vals[1]);
  if (sort_tmp) (void)hipFree(sort_tmp);
  sort_tmp = nullptr;
  sort_tmp_bytes = 0;
  map_cap = 0;
  map_valid = false;
}

void DemEngine::rigid_release()
{
  if (!rigid_) return;
  rigid_->release();
  delete rigid_;
  rigid_ = nullptr;
}

void DemEngine::rigid_rows_ensure()
{
  if (rigid_rows_.ptr) return;   // (registered for capacity growth below: the stride follows the engine's)
  if (cap_ == 0) ensure_capacity(4096);
  rigid_rows_.alloc(sizeof(double), kRigidRows, cap_, stream_);
  rigid_rows_alt_.alloc(sizeof(double), kRigidRows, cap_, stream_);
  per_atom_.push_back(&rigid_rows_);
  per_atom_.push_back(&rigid_rows_alt_);
}

void DemEngine::rigid_molecule_row()
{
  rigid_rows_ensure();
  have_molecule_ = true;
}

void DemEngine::rigid_set_molecule(int n, const int* tags, const int* mol)
{
  if (n < 0 || (n > 0 && (!tags || !mol))) fail("set_molecule: null argument");
  rigid_molecule_row();
  if (!nlocal_ || !n) return;
  std::vector<int> htag(nlocal_);
  std::vector<double> row(nlocal_);
  SF_HIP(hipMemcpyAsync(htag.data(), tag_.ptr, sizeof(int) * nlocal_, hipMemcpyDeviceToHost, stream_));
  double* d_row = rigid_rows_.as<double>() + (size_t)RR_MOL * cap_;
  SF_HIP(hipMemcpyAsync(row.data(), d_row, sizeof(double) * nlocal_, hipMemcpyDeviceToHost, stream_));
  sync();
  std::map<int, int> where;
  for (int i = 0; i < nlocal_; i++) where[htag[i]] = i;
  for (int k = 0; k < n; k++) {
    auto it = where.find(tags[k]);
    if (it == where.end()) fail("set_molecule: no atom with tag %d", tags[k]);
    row[it->second] = (double)mol[k];
  }
  SF_HIP(hipMemcpyAsync(d_row, row.data(), sizeof(double) * nlocal_, hipMemcpyHostToDevice, stream_));
  sync();
  if (rigid_) rigid_->dirty = true;
}

void DemEngine::rigid_define(int bodystyle, int groupbit, const std::vector<int>& groupbits)
{
  if (rigid_) fail("More than one fix rigid/nve");
  if (nranks_ > 1 || have_subdomain_)
    fail("fix rigid/nve needs the whole system on one GPU (one rank, no decomposed domain)");
  if (!roots_) fail("fix rigid/nve is not available with the LDS-staged kernel (SF_LDS)");
  if (bodystyle == 2 && !have_molecule_)
    fail("fix rigid/nve molecule: no molecule IDs (fix ID all property/atom mol, read_data ... fix ID NULL Molecules, or "
         "sf_lammps_set_molecule)");
  rigid_rows_ensure();
  rigid_ = new RigidFix();
  rigid_->bodystyle = bodystyle;
  rigid_->groupbit = groupbit;
  rigid_->groupbits = groupbits;
  use_groups_ = use_groups_ || groupbit != 1 || bodystyle == 1;
}

bool DemEngine::fix_uses_group_bit(int bit) const
{
  if ((have_nve_ && nve_bit_ == bit) || (have_gravity_ && grav_bit_ == bit) || (have_fdrag_ && fdrag_bit_ == bit) ||
      (freeze_bit_ && freeze_bit_ == bit))
    return true;
  for (int k = 0; k < nwalls_; k++)
    if (walls_[k].bit == bit) return true;
  if (rigid_) {
    if (rigid_->groupbit == bit) return true;
    for (int b : rigid_->groupbits)
      if (b == bit) return true;
  }
  return false;
}

void DemEngine::rigid_dirty()
{
  if (rigid_) rigid_->dirty = true;
}

// [3P] FixRigid::setup_bodies, from one download: every sum runs over the atoms of a body in ascending tag order, so the
// bodies do not depend on the order the atoms were handed in
void DemEngine::rigid_setup_bodies()
{
  RigidFix& R = *rigid_;
  if (nranks_ > 1 || have_subdomain_)
    fail("fix rigid/nve needs the whole system on one GPU (one rank, no decomposed domain)");
  const int n = nlocal_;
  std::vector<double4> hx(n), hv(n), hw(n);
  std::vector<int> htag(n), hmask(n);
  std::vector<double> hmol(n, 0.0);
  if (n) {
    SF_HIP(hipMemcpyAsync(hx.data(), xr_[cur_].ptr, sizeof(double4) * n, hipMemcpyDeviceToHost, stream_));
    SF_HIP(hipMemcpyAsync(hv.data(), vm_[cur_].ptr, sizeof(double4) * n, hipMemcpyDeviceToHost, stream_));
    SF_HIP(hipMemcpyAsync(hw.data(), om_[cur_].ptr, sizeof(double4) * n, hipMemcpyDeviceToHost, stream_));
    SF_HIP(hipMemcpyAsync(htag.data(), tag_.ptr, sizeof(int) * n, hipMemcpyDeviceToHost, stream_));
    SF_HIP(hipMemcpyAsync(hmask.data(), mask_.ptr, sizeof(int) * n, hipMemcpyDeviceToHost, stream_));
    SF_HIP(hipMemcpyAsync(hmol.data(), rigid_rows_.as<double>() + (size_t)RR_MOL * cap_, sizeof(double) * n,
                          hipMemcpyDeviceToHost, stream_));
  }
  sync();
  // which body an atom is in: a provisional key, then the bodies are numbered by the smallest tag they hold
  std::vector<long long> key(n, -1);
  for (int i = 0; i < n; i++) {
    if (!(hmask[i] & R.groupbit)) continue;
    if (R.bodystyle == 0) key[i] = 0;
    else if (R.bodystyle == 1) {
      for (size_t g = 0; g < R.groupbits.size(); g++)
        if (hmask[i] & R.groupbits[g]) {
          if (key[i] >= 0) fail("fix rigid/nve group: atom %d is in more than one of the body groups", htag[i]);
          key[i] = (long long)g;
        }
    } else
      key[i] = (long long)hmol[i];
    if (key[i] >= 0 && have_nve_ && (hmask[i] & nve_bit_))
      fail("fix rigid/nve: atom %d is also in the group of fix nve/sphere (it would be integrated twice)", htag[i]);
  }
  std::map<long long, std::vector<int>> members;   // key -> atoms
  for (int i = 0; i < n; i++)
    if (key[i] >= 0) members[key[i]].push_back(i);
  std::vector<std::vector<int>> bodies;
  for (auto& m : members) {
    std::sort(m.second.begin(), m.second.end(), [&](int a, int b) { return htag[a] < htag[b]; });
    bodies.push_back(m.second);
  }
  std::sort(bodies.begin(), bodies.end(),
            [&](const std::vector<int>& a, const std::vector<int>& b) { return htag[a[0]] < htag[b[0]]; });
  const int nb = (int)bodies.size();
  if (nb == 0) fail("fix rigid/nve: no atoms in any rigid body");
  double prd[3];
  for (int k = 0; k < 3; k++) prd[k] = boxhi_[k] - boxlo_[k];

  std::vector<double> bs((size_t)kBodyFields * nb, 0.0);
  auto B = [&](int f, int b) -> double& { return bs[(size_t)f * nb + b]; };
  std::vector<double> rows((size_t)kRigidRows * n, 0.0);
  for (int i = 0; i < n; i++) {
    rows[(size_t)RR_BODY * n + i] = -1.0;
    rows[(size_t)RR_MBODY * n + i] = hv[i].w;   // no body: the atom's own mass
    rows[(size_t)RR_MOL * n + i] = hmol[i];
  }
  R.natoms.assign(nb, 0);
  R.off.assign(nb + 1, 0);
  std::vector<double> ux, uy, uz;
  for (int b = 0; b < nb; b++) {
    const std::vector<int>& at = bodies[b];
    const int na = (int)at.size();
    R.natoms[b] = na;
    R.off[b + 1] = R.off[b] + na;
    // unwrapped positions: minimum image relative to the body's lowest-tag atom
    ux.assign(na, 0.0); uy.assign(na, 0.0); uz.assign(na, 0.0);
    const double4 x0 = hx[at[0]];
    double lo3[3] = {0, 0, 0}, hi3[3] = {0, 0, 0};
    for (int a = 0; a < na; a++) {
      double d[3] = {hx[at[a]].x - x0.x, hx[at[a]].y - x0.y, hx[at[a]].z - x0.z};
      for (int k = 0; k < 3; k++) {
        if (periodic_[k]) d[k] -= prd[k] * std::nearbyint(d[k] / prd[k]);
        lo3[k] = std::min(lo3[k], d[k]);
        hi3[k] = std::max(hi3[k], d[k]);
      }
      ux[a] = x0.x + d[0]; uy[a] = x0.y + d[1]; uz[a] = x0.z + d[2];
    }
    for (int k = 0; k < 3; k++)
      if (periodic_[k] && hi3[k] - lo3[k] > 0.5 * prd[k])
        fail("fix rigid/nve: the body of atom %d is wider than half the periodic box in %c", htag[at[0]], "xyz"[k]);
    double M = 0.0, xc[3] = {0, 0, 0}, vc[3] = {0, 0, 0};
    for (int a = 0; a < na; a++) {
      const double m = hv[at[a]].w;
      M += m;
      xc[0] += m * ux[a]; xc[1] += m * uy[a]; xc[2] += m * uz[a];
      vc[0] += m * hv[at[a]].x; vc[1] += m * hv[at[a]].y; vc[2] += m * hv[at[a]].z;
    }
    for (int k = 0; k < 3; k++) {
      xc[k] /= M;
      vc[k] /= M;
    }
    double T[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int a = 0; a < na; a++) {
      const double m = hv[at[a]].w, r = hx[at[a]].w;
      const double dx = ux[a] - xc[0], dy = uy[a] - xc[1], dz = uz[a] - xc[2];
      const double sph = 0.4 * m * r * r;
      T[0][0] += m * (dy * dy + dz * dz) + sph;
      T[1][1] += m * (dx * dx + dz * dz) + sph;
      T[2][2] += m * (dx * dx + dy * dy) + sph;
      T[0][1] -= m * dx * dy;
      T[0][2] -= m * dx * dz;
      T[1][2] -= m * dy * dz;
    }
    T[1][0] = T[0][1]; T[2][0] = T[0][2]; T[2][1] = T[1][2];
    double I[3], E[3][3];
    jacobi3(T, I, E);
    double ex[3] = {E[0][0], E[1][0], E[2][0]}, ey[3] = {E[0][1], E[1][1], E[2][1]}, ez[3] = {E[0][2], E[1][2], E[2][2]};
    const double imax = std::max(I[0], std::max(I[1], I[2]));
    for (int k = 0; k < 3; k++)
      if (I[k] < 1.0e-7 * imax) I[k] = 0.0;
    // right-handed triple
    const double cx[3] = {ex[1] * ey[2] - ex[2] * ey[1], ex[2] * ey[0] - ex[0] * ey[2], ex[0] * ey[1] - ex[1] * ey[0]};
    if (cx[0] * ez[0] + cx[1] * ez[1] + cx[2] * ez[2] < 0.0)
      for (int k = 0; k < 3; k++) ez[k] = -ez[k];
    double q[4];
    quat_of_axes(ex, ey, ez, q);
    // (the axes the kernels use are the ones the quaternion gives back)
    ex[0] = q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3]; ex[1] = 2.0 * (q[1] * q[2] + q[0] * q[3]); ex[2] = 2.0 * (q[1] * q[3] - q[0] * q[2]);
    ey[0] = 2.0 * (q[1] * q[2] - q[0] * q[3]); ey[1] = q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3]; ey[2] = 2.0 * (q[2] * q[3] + q[0] * q[1]);
    ez[0] = 2.0 * (q[1] * q[3] + q[0] * q[2]); ez[1] = 2.0 * (q[2] * q[3] - q[0] * q[1]); ez[2] = q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3];
    double L[3] = {0, 0, 0};
    for (int a = 0; a < na; a++) {
      const int i = at[a];
      const double m = hv[i].w, r = hx[i].w;
      const double d[3] = {ux[a] - xc[0], uy[a] - xc[1], uz[a] - xc[2]};
      rows[(size_t)RR_BODY * n + i] = (double)b;
      rows[(size_t)(RR_DISP + 0) * n + i] = d[0] * ex[0] + d[1] * ex[1] + d[2] * ex[2];
      rows[(size_t)(RR_DISP + 1) * n + i] = d[0] * ey[0] + d[1] * ey[1] + d[2] * ey[2];
      rows[(size_t)(RR_DISP + 2) * n + i] = d[0] * ez[0] + d[1] * ez[1] + d[2] * ez[2];
      rows[(size_t)RR_MBODY * n + i] = M;
      const double sph = 0.4 * m * r * r;
      L[0] += m * (d[1] * hv[i].z - d[2] * hv[i].y) + sph * hw[i].x;
      L[1] += m * (d[2] * hv[i].x - d[0] * hv[i].z) + sph * hw[i].y;
      L[2] += m * (d[0] * hv[i].y - d[1] * hv[i].x) + sph * hw[i].z;
    }
    // omega, conjqm = 2 q (x) (0, R^T angmom)
    const double Lb[3] = {L[0] * ex[0] + L[1] * ex[1] + L[2] * ex[2], L[0] * ey[0] + L[1] * ey[1] + L[2] * ey[2],
                          L[0] * ez[0] + L[1] * ez[1] + L[2] * ez[2]};
    double wb[3];
    for (int k = 0; k < 3; k++) wb[k] = I[k] == 0.0 ? 0.0 : Lb[k] / I[k];
    for (int k = 0; k < 3; k++) {
      B(BF_XCM + k, b) = xc[k];
      B(BF_VCM + k, b) = vc[k];
      B(BF_ANGMOM + k, b) = L[k];
      B(BF_OMEGA + k, b) = wb[0] * ex[k] + wb[1] * ey[k] + wb[2] * ez[k];
      B(BF_INERTIA + k, b) = I[k];
      B(BF_EX + k, b) = ex[k];
      B(BF_EX + 3 + k, b) = ey[k];
      B(BF_EX + 6 + k, b) = ez[k];
    }
    for (int k = 0; k < 4; k++) B(BF_QUAT + k, b) = q[k];
    B(BF_CONJQM + 0, b) = 2.0 * (-q[1] * Lb[0] - q[2] * Lb[1] - q[3] * Lb[2]);
    B(BF_CONJQM + 1, b) = 2.0 * (q[0] * Lb[0] + q[2] * Lb[2] - q[3] * Lb[1]);
    B(BF_CONJQM + 2, b) = 2.0 * (q[0] * Lb[1] + q[3] * Lb[0] - q[1] * Lb[2]);
    B(BF_CONJQM + 3, b) = 2.0 * (q[0] * Lb[2] + q[1] * Lb[1] - q[2] * Lb[0]);
    B(BF_MASS, b) = M;
  }
  // upload: the per-atom rows in the current atom order, the bodies, the shape of the reduction
  for (int r = 0; r < kRigidRows && n; r++)
    SF_HIP(hipMemcpyAsync(rigid_rows_.as<double>() + (size_t)r * cap_, rows.data() + (size_t)r * n, sizeof(double) * n,
                          hipMemcpyHostToDevice, stream_));
  R.nbody = nb;
  R.nin = R.off[nb];
  std::vector<int> small, large_id, large_c0, large_nc, ch_body, ch_first, ch_end;
  for (int b = 0; b < nb; b++) {
    if (R.natoms[b] <= kRigidSmall) {
      small.push_back(b);
      continue;
    }
    large_id.push_back(b);
    large_c0.push_back((int)ch_body.size());
    for (int q = R.off[b]; q < R.off[b + 1]; q += kRigidChunk) {
      ch_body.push_back(b);
      ch_first.push_back(q);
      ch_end.push_back(std::min(q + kRigidChunk, R.off[b + 1]));
    }
    large_nc.push_back((int)ch_body.size() - large_c0.back());
  }
  R.nsmall = (int)small.size();
  R.nlarge = (int)large_id.size();
  R.nchunks = (int)ch_body.size();
  std::vector<int> large(large_id), chunk(ch_body);
  large.insert(large.end(), large_c0.begin(), large_c0.end());
  large.insert(large.end(), large_nc.begin(), large_nc.end());
  chunk.insert(chunk.end(), ch_first.begin(), ch_first.end());
  chunk.insert(chunk.end(), ch_end.begin(), ch_end.end());
  dev_upload(R.bs, bs, stream_);
  dev_upload(R.d_off, R.off, stream_);
  dev_upload(R.d_small, small, stream_);
  dev_upload(R.d_large, large, stream_);
  dev_upload(R.d_chunk, chunk, stream_);
  dev_free(R.d_part);
  SF_HIP(hipMalloc(&R.d_part, sizeof(double) * 6 * std::max(R.nchunks, 1)));
  sync();   // (the host vectors go out of scope)
  R.dirty = false;
  R.map_valid = false;
  R.force_stale = true;   // (fcm / torque of the new bodies are 0 until a reduction)
}

// the body -> atom map of the current atom order: a stable sort of the atom indices by body (rebuilt with every list)
void DemEngine::rigid_map_rebuild()
{
  if (!rigid_ || rigid_->dirty || !rigid_->nbody || !nlocal_) return;
  RigidFix& R = *rigid_;
  if (R.map_cap < cap_) {
    for (int k = 0; k < 2; k++) {
      dev_free(R.keys[k]);
      dev_free(R.vals[k]);
      SF_HIP(hipMalloc(&R.keys[k], sizeof(unsigned) * cap_));
      SF_HIP(hipMalloc(&R.vals[k], sizeof(int) * cap_));
    }
    R.map_cap = cap_;
  }
  k_rigid_keys<<<div_up(nlocal_, 256), 256, 0, stream_>>>(rigid_rows_.as<double>() + (size_t)RR_BODY * cap_, nlocal_, R.nbody,
                                                         R.keys[0], R.vals[0]);
  int bits = 1;
  while (bits < 32 && (1ll << bits) <= (long long)R.nbody) bits++;
  sort_pairs_u32(R.sort_tmp, R.sort_tmp_bytes, R.keys[0], R.keys[1], R.vals[0], R.vals[1], nlocal_, bits, stream_);
  SF_HIP(hipGetLastError());
  R.map_valid = true;
}

namespace {
RigidView view_of(const RigidFix& R, const double* rows, size_t cap, int* flags)
{
  RigidView V;
  V.bs = R.bs;
  V.nbody = R.nbody;
  V.rows = rows;
  V.cap = cap;
  V.map = R.vals[1];
  V.off = R.d_off;
  V.flags = flags;
  return V;
}
}  // namespace

// fcm, torque of every body from the per-atom force / torque of the evaluation just queued
void DemEngine::rigid_reduce(int kstep)
{
  RigidFix& R = *rigid_;
  if (!R.map_valid) fail("fix rigid/nve: the body -> atom map is missing (internal error)");
  const RigidView V = view_of(R, rigid_rows_.as<double>(), cap_, d_flags_);
  if (R.nsmall)
    k_rigid_reduce_small<<<div_up(R.nsmall, 256), 256, 0, stream_>>>(V, R.d_small, R.nsmall, force_.as<double4>(),
                                                                     torque_.as<double4>(), kstep);
  if (R.nlarge) {
    k_rigid_partials<<<R.nchunks, kRigidChunk, 0, stream_>>>(V, R.d_chunk, R.nchunks, force_.as<double4>(),
                                                            torque_.as<double4>(), R.d_part, kstep);
    k_rigid_reduce_large<<<R.nlarge, 256, 0, stream_>>>(V, R.d_large, R.nlarge, R.d_part, kstep);
  }
  SF_HIP(hipGetLastError());
  R.force_stale = false;
}

void DemEngine::rigid_integrate(int kstep, bool do_final, bool do_initial)
{
  RigidFix& R = *rigid_;
  const RigidView V = view_of(R, rigid_rows_.as<double>(), cap_, d_flags_);
  const double3 lo = {boxlo_[0], boxlo_[1], boxlo_[2]};
  const double3 prd = {boxhi_[0] - boxlo_[0], boxhi_[1] - boxlo_[1], boxhi_[2] - boxlo_[2]};
  const int3 per = {periodic_[0], periodic_[1], periodic_[2]};
  k_rigid_integrate<<<div_up(R.nbody, 64), 64, 0, stream_>>>(V, dt_, do_final ? 1 : 0, do_initial ? 1 : 0, kstep, lo, prd, per);
  SF_HIP(hipGetLastError());
}

void DemEngine::rigid_writeback(int in_buf, int out_buf, int kstep, bool do_final, bool do_initial)
{
  RigidFix& R = *rigid_;
  if (!nlocal_) return;
  const RigidView V = view_of(R, rigid_rows_.as<double>(), cap_, d_flags_);
  WritebackArgs A;
  A.xi = xr_[in_buf].as<double4>();
  A.vi = vm_[in_buf].as<double4>();
  A.wi = om_[in_buf].as<double4>();
  A.xo = xr_[out_buf].as<double4>();
  A.vo = vm_[out_buf].as<double4>();
  A.wo = om_[out_buf].as<double4>();
  A.force = force_.as<double4>();
  A.torque = torque_.as<double4>();
  A.xhold = xhold_.as<double>();
  A.mask = use_groups_ ? mask_.as<int>() : nullptr;
  A.nlocal = nlocal_;
  A.have_nve = have_nve_ ? 1 : 0;
  A.nve_bit = nve_bit_;
  A.do_final = do_final ? 1 : 0;
  A.do_initial = do_initial ? 1 : 0;
  A.kstep = kstep;
  A.dt = dt_;
  A.trigger_sq = (0.5 * skin_) * (0.5 * skin_);
  for (int k = 0; k < 3; k++) {
    A.lo[k] = boxlo_[k];
    A.prd[k] = boxhi_[k] - boxlo_[k];
    A.per[k] = periodic_[k];
  }
  k_rigid_writeback<<<div_up(nlocal_, 256), 256, 0, stream_>>>(V, A);
  SF_HIP(hipGetLastError());
}

// the bodies exist and the map matches the atom order (setup, and whenever atoms changed behind the fix's back).  New
// bodies carry no fcm / torque: with `reduce` they are summed from the forces stored by the last evaluation (the atoms
// are still in that order), whoever derived the bodies -- a step or a query in between
void DemEngine::rigid_prepare(bool reduce)
{
  RigidFix& R = *rigid_;
  if (R.dirty) rigid_setup_bodies();
  if (!R.map_valid) rigid_map_rebuild();
  if (reduce && R.force_stale) rigid_reduce(INT_MIN);
}

// after the setup force evaluation (mode 2): fcm / torque, then the records into the other buffer with v, omega of the
// body atoms set by their bodies ([3P] FixRigid::setup -> set_v)
void DemEngine::rigid_after_setup_force(int in_buf)
{
  rigid_reduce(0);
  rigid_writeback(in_buf, in_buf ^ 1, 0, false, false);
}

// DemEngine::run with the fix: the same queue / trigger / rebuild loop, four kernels per sub-step
void DemEngine::run_rigid(int nsteps)
{
  run_base_step_ = nsteps_;
  choose_kernel();
  reset_flag(F_TRIGGER, INT_MAX);
  rigid_prepare(true);
  // initial half of the first step, in place ([3P] FixRigidNVE::initial_integrate; free atoms: FixNVESphere's)
  rigid_integrate(-1, false, true);
  rigid_writeback(cur_, cur_, -1, false, true);
  int k = 0;
  SF_HIP(hipEventRecord(ev0_, stream_));
  while (k < nsteps) {
    const int base = cur_;
    prof_used_ = 0;
    predict_.overshoot = false;
    const int end = k + predict_.chunk(run_base_step_ + k, nsteps - k);
    for (int s = k; s < end; s++) {
      const int in_buf = (base + (s - k)) & 1;
      const bool last = s == nsteps - 1;
      launch_substep(in_buf, 1, s);   // (forces only: the RIGID instantiation stores force / torque and no records)
      rigid_reduce(s);
      rigid_integrate(s, true, !last);
      rigid_writeback(in_buf, in_buf ^ 1, s, true, !last);
    }
    read_flags();
    const int trig = h_flags_[F_TRIGGER];
    if (profiling_) {
      harvest_profile(trig);
      prof_used_ = 0;
    }
    if (trig == INT_MAX) {
      cur_ = (base + (end - k)) & 1;
      k = end;
    } else {
      const int done = trig + 1 - k;
      cur_ = (base + done) & 1;
      k = trig + 1;
      InRunGuard guard(*this);
      rebuild();   // (ends with rigid_map_rebuild)
      guard.release();
      predict_.rebuilt(run_base_step_ + k);
    }
  }
  SF_HIP(hipEventRecord(ev1_, stream_));
  sync();
  float ms = 0.f;
  SF_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
  last_substep_ms_ = ms / nsteps;
  nsteps_ += nsteps;
}

int DemEngine::rigid_nbody()
{
  if (!rigid_) return 0;
  // (before the first setup there are no forces yet: setup() reduces after its own evaluation)
  if (rigid_->dirty && nlocal_) rigid_prepare(setup_done_);
  return rigid_->nbody;
}

void DemEngine::rigid_get(int* natoms, double* fields)
{
  if (!rigid_) fail("sf_lammps_get_rigid: no fix rigid/nve");
  const int nb = rigid_nbody();
  if (!nb) return;
  sync();
  SF_HIP(hipMemcpy(fields, rigid_->bs, sizeof(double) * (size_t)kBodyFields * nb, hipMemcpyDeviceToHost));
  for (int b = 0; b < nb; b++) natoms[b] = rigid_->natoms[b];
}

}  // namespace sf
