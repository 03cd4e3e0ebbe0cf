"""A NumPy model of fix rigid/nve for bodies of spheres under external per-atom forces and gravity (no contacts): the rules
of DESIGN.md section 11 restated in float64 (or any NumPy float type: the self-checks run it in np.longdouble too).
Test infrastructure: written from the rules, not from the HIP code; vectorised over the bodies.

Atoms are given in any order; `body[i]` is the body of atom i (-1: a free atom advanced by fix nve/sphere).  Bodies are
numbered by the caller.  Every per-body sum runs over the atoms in the order they were given -- summation order is the
engine's freedom, and running the model on two orders measures what that freedom is worth."""
import numpy as np


def _jacobi(a, dtype):
    """eigenvalues and eigenvectors (columns) of a symmetric 3 x 3 matrix by cyclic Jacobi rotations"""
    a = np.array(a, dtype=dtype)
    v = np.eye(3, dtype=dtype)
    one, two = dtype(1), dtype(2)
    for _ in range(100):
        off = abs(a[0, 1]) + abs(a[0, 2]) + abs(a[1, 2])
        if off == 0 or off <= np.finfo(dtype).tiny + np.finfo(dtype).eps ** 2 * np.trace(abs(a)):
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if a[p, q] == 0:
                    continue
                theta = (a[q, q] - a[p, p]) / (two * a[p, q])
                t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                J = np.eye(3, dtype=dtype)
                J[p, p] = J[q, q] = c
                J[p, q] = s
                J[q, p] = -s
                a = J.T @ a @ J
                v = v @ J
    return np.diag(a).copy(), v


def _axes(q):
    """rows ex, ey, ez of the bodies' principal axes in the space frame from quaternions [nb, 4] (w x y z)"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    ex = np.stack([w * w + x * x - y * y - z * z, 2 * (x * y + w * z), 2 * (x * z - w * y)], axis=1)
    ey = np.stack([2 * (x * y - w * z), w * w - x * x + y * y - z * z, 2 * (y * z + w * x)], axis=1)
    ez = np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), w * w - x * x - y * y + z * z], axis=1)
    return ex, ey, ez


def _quat_from_axes(ex, ey, ez, dtype):
    """one body: the unit quaternion whose rotation matrix has the columns ex, ey, ez"""
    R = np.stack([ex, ey, ez], axis=1)   # columns
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    sq = [dtype(0.25) * (tr + 1), dtype(0.25) * (1 + R[0, 0] - R[1, 1] - R[2, 2]),
          dtype(0.25) * (1 - R[0, 0] + R[1, 1] - R[2, 2]), dtype(0.25) * (1 - R[0, 0] - R[1, 1] + R[2, 2])]
    k = int(np.argmax(sq))
    q = np.zeros(4, dtype=dtype)
    q[k] = np.sqrt(sq[k])
    d = 4 * q[k]
    if k == 0:
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) / d, (R[0, 2] - R[2, 0]) / d, (R[1, 0] - R[0, 1]) / d
    elif k == 1:
        q[0], q[2], q[3] = (R[2, 1] - R[1, 2]) / d, (R[0, 1] + R[1, 0]) / d, (R[0, 2] + R[2, 0]) / d
    elif k == 2:
        q[0], q[1], q[3] = (R[0, 2] - R[2, 0]) / d, (R[0, 1] + R[1, 0]) / d, (R[1, 2] + R[2, 1]) / d
    else:
        q[0], q[1], q[2] = (R[1, 0] - R[0, 1]) / d, (R[0, 2] + R[2, 0]) / d, (R[1, 2] + R[2, 1]) / d
    return q / np.sqrt(np.sum(q * q))


def _qmul_vec(q, b):
    """q (x) (0, b) for arrays [nb, 4], [nb, 3]"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([-x * b[:, 0] - y * b[:, 1] - z * b[:, 2], w * b[:, 0] + y * b[:, 2] - z * b[:, 1],
                     w * b[:, 1] + z * b[:, 0] - x * b[:, 2], w * b[:, 2] + x * b[:, 1] - y * b[:, 0]], axis=1)


def _qinv_mul_xyz(q, p):
    """vector part of q^-1 (x) p for unit quaternions"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([-x * p[:, 0] + w * p[:, 1] + z * p[:, 2] - y * p[:, 3],
                     -y * p[:, 0] - z * p[:, 1] + w * p[:, 2] + x * p[:, 3],
                     -z * p[:, 0] + y * p[:, 1] - x * p[:, 2] + w * p[:, 3]], axis=1)


_PERM = {1: ((1, -1), (0, 1), (3, 1), (2, -1)), 2: ((2, -1), (3, -1), (0, 1), (1, 1)), 3: ((3, -1), (2, 1), (1, -1), (0, 1))}


def _kmul(k, q):
    return np.stack([s * q[:, j] for j, s in _PERM[k]], axis=1)


class RigidModel:
    def __init__(self, x, v, omega, radius, mass, body, boxlo, boxhi, periodic, dt, dtype=np.float64, tag=None):
        T = self.T = dtype
        self.tag = np.arange(1, len(body) + 1) if tag is None else np.asarray(tag)
        self.x = np.array(x, dtype=T)
        self.v = np.array(v, dtype=T)
        self.w = np.array(omega, dtype=T)
        self.r = np.array(radius, dtype=T)
        self.m = np.array(mass, dtype=T)
        self.body = np.asarray(body, dtype=np.int64)
        self.lo = np.array(boxlo, dtype=T)
        self.prd = np.array(boxhi, dtype=T) - self.lo
        self.per = np.asarray(periodic, dtype=bool)
        self.dt = T(dt)
        self.nb = int(self.body.max()) + 1 if self.body.size and self.body.max() >= 0 else 0
        self.inb = self.body >= 0
        self.f = np.zeros_like(self.x)
        self.setup()

    def _bsum(self, vals):
        out = np.zeros((self.nb,) + vals.shape[1:], dtype=self.T)
        np.add.at(out, self.body[self.inb], vals[self.inb])   # (unbuffered: element by element in the given order)
        return out

    def setup(self):
        T, nb = self.T, self.nb
        b = np.where(self.inb, self.body, 0)
        # unwrap by minimum image relative to the body's lowest-tag atom
        first = np.full(nb, -1)
        for i in np.nonzero(self.inb)[0][np.argsort(-self.tag[self.inb], kind="stable")]:
            first[self.body[i]] = i
        d = self.x - self.x[first[b]]
        d = d - np.where(self.per, self.prd * np.rint(d / self.prd), 0)
        xu = self.x[first[b]] + d
        m1 = self.m[:, None]
        self.M = self._bsum(self.m)
        self.xcm = self._bsum(m1 * xu) / self.M[:, None]
        self.vcm = self._bsum(m1 * self.v) / self.M[:, None]
        D = xu - self.xcm[b]
        sph = T(0.4) * self.m * self.r * self.r
        ten = np.zeros((self.x.shape[0], 3, 3), dtype=T)
        ten[:, 0, 0] = self.m * (D[:, 1] ** 2 + D[:, 2] ** 2) + sph
        ten[:, 1, 1] = self.m * (D[:, 0] ** 2 + D[:, 2] ** 2) + sph
        ten[:, 2, 2] = self.m * (D[:, 0] ** 2 + D[:, 1] ** 2) + sph
        ten[:, 0, 1] = ten[:, 1, 0] = -self.m * D[:, 0] * D[:, 1]
        ten[:, 0, 2] = ten[:, 2, 0] = -self.m * D[:, 0] * D[:, 2]
        ten[:, 1, 2] = ten[:, 2, 1] = -self.m * D[:, 1] * D[:, 2]
        ten = self._bsum(ten)
        self.I = np.zeros((nb, 3), dtype=T)
        self.q = np.zeros((nb, 4), dtype=T)
        for k in range(nb):
            I, E = _jacobi(ten[k], T)
            ex, ey, ez = E[:, 0], E[:, 1], E[:, 2]
            if np.dot(np.cross(ex, ey), ez) < 0:
                ez = -ez
            I[I < T(1e-7) * I.max()] = 0
            self.I[k] = I
            self.q[k] = _quat_from_axes(ex, ey, ez, T)
        ex, ey, ez = _axes(self.q)
        self.disp = np.stack([np.sum(D * ex[b], axis=1), np.sum(D * ey[b], axis=1), np.sum(D * ez[b], axis=1)], axis=1)
        L = self._bsum(m1 * np.cross(D, self.v) + sph[:, None] * self.w)
        Lb = np.stack([np.sum(L * ex, axis=1), np.sum(L * ey, axis=1), np.sum(L * ez, axis=1)], axis=1)
        self.p = 2 * _qmul_vec(self.q, Lb)
        self.fcm = np.zeros((nb, 3), dtype=T)
        self.tq = np.zeros((nb, 3), dtype=T)
        self._derive()
        self._set_v()

    def _R(self, vec_body):
        ex, ey, ez = _axes(self.q)
        return ex * vec_body[:, 0:1] + ey * vec_body[:, 1:2] + ez * vec_body[:, 2:3]

    def _derive(self):
        ex, ey, ez = _axes(self.q)
        Lb = self.T(0.5) * _qinv_mul_xyz(self.q, self.p)
        self.L = self._R(Lb)
        with np.errstate(divide="ignore", invalid="ignore"):
            wb = np.where(self.I == 0, 0, Lb / np.where(self.I == 0, 1, self.I))
        self.om = self._R(wb)

    def _delta(self):
        b = np.where(self.inb, self.body, 0)
        ex, ey, ez = _axes(self.q)
        return ex[b] * self.disp[:, 0:1] + ey[b] * self.disp[:, 1:2] + ez[b] * self.disp[:, 2:3]

    def _set_v(self, place=False):
        b = np.where(self.inb, self.body, 0)
        D = self._delta()
        i = self.inb
        if place:
            xn = self.xcm[b] + D
            xn = xn + np.where(self.per & (xn < self.lo), self.prd, 0) - np.where(self.per & (xn >= self.lo + self.prd), self.prd, 0)
            self.x[i] = xn[i]
        self.v[i] = (np.cross(self.om[b], D) + self.vcm[b])[i]
        self.w[i] = self.om[b][i]

    def _forces(self, fext, g):
        self.f = np.asarray(fext, dtype=self.T) + self.m[:, None] * np.asarray(g, dtype=self.T)
        if self.nb:
            self.fcm = self._bsum(self.f)
            self.tq = self._bsum(np.cross(self._delta(), self.f))

    def _kick(self):
        dtf = self.T(0.5) * self.dt
        self.vcm = self.vcm + dtf * self.fcm / self.M[:, None]
        ex, ey, ez = _axes(self.q)
        tb = np.stack([np.sum(self.tq * ex, axis=1), np.sum(self.tq * ey, axis=1), np.sum(self.tq * ez, axis=1)], axis=1)
        self.p = self.p + dtf * 2 * _qmul_vec(self.q, tb)

    def _rotate(self, k, dt):
        kq, kp = _kmul(k, self.q), _kmul(k, self.p)
        phi = np.sum(self.p * kq, axis=1)
        Ik = self.I[:, k - 1]
        phi = np.where(Ik == 0, 0, phi / (4 * np.where(Ik == 0, 1, Ik)))
        c, s = np.cos(dt * phi)[:, None], np.sin(dt * phi)[:, None]
        self.p = c * self.p + s * kp
        self.q = c * self.q + s * kq

    def _free_kick(self):
        fr = ~self.inb
        dtf = self.T(0.5) * self.dt
        self.v[fr] += (dtf / self.m[fr])[:, None] * self.f[fr]
        # (no torque on a free sphere in this model: its spin stays)

    def setup_forces(self, fext, g):
        self._forces(fext, g)

    def step(self, n, fext, g):
        """n steps of velocity Verlet; the forces of the current positions must be there (setup_forces, or a step)"""
        half = self.T(0.5) * self.dt
        fr = ~self.inb
        for _ in range(n):
            # initial integrate
            if self.nb:
                self._kick()
                self.xcm = self.xcm + self.dt * self.vcm
                for k, t in ((3, half), (2, half), (1, self.dt), (2, half), (3, half)):
                    self._rotate(k, t)
                self.q = self.q / np.sqrt(np.sum(self.q * self.q, axis=1))[:, None]
                self.xcm = (self.xcm + np.where(self.per & (self.xcm < self.lo), self.prd, 0)
                            - np.where(self.per & (self.xcm >= self.lo + self.prd), self.prd, 0))
                self._derive()
                self._set_v(place=True)
            self._free_kick()
            self.x[fr] += self.dt * self.v[fr]
            # forces, final integrate
            self._forces(fext, g)
            if self.nb:
                self._kick()
                self._derive()
                self._set_v()
            self._free_kick()

    def rotational_energy(self):
        ex, ey, ez = _axes(self.q)
        Lb = np.stack([np.sum(self.L * ex, axis=1), np.sum(self.L * ey, axis=1), np.sum(self.L * ez, axis=1)], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return 0.5 * np.sum(np.where(self.I == 0, 0, Lb * Lb / np.where(self.I == 0, 1, self.I)), axis=1)

    def inertia_space(self):
        """the inertia tensors in the space frame, [nb, 3, 3]: independent of how the principal axes are numbered"""
        ex, ey, ez = _axes(self.q)
        E = np.stack([ex, ey, ez], axis=2)
        return np.einsum("bik,bk,bjk->bij", E, self.I, E)
