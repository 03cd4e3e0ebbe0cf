"""The NumPy statement of the unwrapped-coordinate keywords: the unwrapped coordinate, the image
bookkeeping by the rule of the rebuild's wrap kernel, compute displace/atom, the mean squared displacement (what compute
reduce avesq over its columns gives; with a centre of mass taken off, which no style here does yet), compute com.
Every function takes and returns float64 / int32 arrays; nothing here is fused, so `x + ix * L` has the bits the device's
unmap() has."""
import numpy as np


def unmap(x, image, prd):
    """x + image * prd per component ([3P] Domain::unmap for an orthogonal box): the product, then the sum"""
    x = np.asarray(x, np.float64)
    return x + np.asarray(image, np.float64) * np.asarray(prd, np.float64)


def wrap(x, image, lo, hi, periodic):
    """One pass of the wrap the rebuild applies ([3P] Domain::pbc as the engine's kernel has it): below lo a box length is
    added and the count goes down by one, at or above hi one is taken off (never to below lo) and the count goes up by
    one.  Returns (x, image), new arrays.  At most one box length per dimension per pass, as the kernel"""
    x = np.array(x, np.float64)
    image = np.array(image, np.int32)
    for k in range(3):
        if not periodic[k]:
            continue
        prd = hi[k] - lo[k]
        below = x[:, k] < lo[k]
        x[below, k] += prd
        image[below, k] -= 1
        above = x[:, k] >= hi[k]
        x[above, k] -= prd
        x[above & (x[:, k] < lo[k]), k] = lo[k]
        image[above, k] += 1
    return x, image


def displace(xu, x0, in_group=None):
    """the four columns of compute displace/atom: dx dy dz and sqrt(dx^2 + dy^2 + dz^2); atoms outside the group read 0"""
    d = np.asarray(xu, np.float64) - np.asarray(x0, np.float64)
    if in_group is not None:
        d = np.where(np.asarray(in_group, bool)[:, None], d, 0.0)
    return np.column_stack([d, np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])])


def com(xu, mass, in_group=None):
    """sum m xu / sum m over the group ([3P] Group::xcm); zeros for a group of no atoms"""
    xu = np.asarray(xu, np.float64)
    m = np.asarray(mass, np.float64)
    if in_group is not None:
        xu, m = xu[np.asarray(in_group, bool)], m[np.asarray(in_group, bool)]
    if m.size == 0 or m.sum() <= 0.0:
        return np.zeros(3)
    return (xu * m[:, None]).sum(axis=0) / m.sum()


def msd(xu, x0, in_group=None, cm=None):
    """the mean squared displacement: the group means of dx^2, dy^2, dz^2 and of their sum ([3P] ComputeMSD's four values).
    cm: the group's centre of mass now, as LAMMPS' `com yes` takes it off -- x0 is then relative to the centre of mass of ITS
    moment"""
    xu = np.asarray(xu, np.float64)
    x0 = np.asarray(x0, np.float64)
    if in_group is not None:
        xu, x0 = xu[np.asarray(in_group, bool)], x0[np.asarray(in_group, bool)]
    if xu.shape[0] == 0:
        return np.zeros(4)
    d = (xu - (np.zeros(3) if cm is None else np.asarray(cm, np.float64))) - x0
    s = d * d
    return np.append(s.sum(axis=0), ((s[:, 0] + s[:, 1]) + s[:, 2]).sum()) / xu.shape[0]


def msd_terms(xu, x0, cm=None):
    """sum over the atoms of |term| for each of the four values of msd(), before the division: the scale a bound on the
    order of the additions is relative to (the terms are squares: the sum itself)"""
    d = (np.asarray(xu, np.float64) - (np.zeros(3) if cm is None else np.asarray(cm, np.float64))) - np.asarray(x0, np.float64)
    s = d * d
    return np.append(s.sum(axis=0), s.sum())
