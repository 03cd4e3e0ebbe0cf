"""The rules of `compute cluster/atom CUT [surface no|yes] [size no|yes]` and `compute cluster/stats CID`
in NumPy and plain Python: brute force over all pairs for the links, a breadth-first search for the components.  Written from
the rules, not from the engine's code; tests/test_cluster_model.py holds it to answers worked out by hand and
tests/test_cluster_gpu.py holds the engine to it.  Every value is an integer, so the engine must equal this model with ==."""
from collections import deque

import numpy as np

from tests import nbr_model as nm


def grid_cutoff(cut, surface=False, rmax=0.0):
    """the cutoff of the grid the engine walks, which a periodic box length must be at least twice of"""
    return np.float64(2.0) * np.float64(rmax) + np.float64(cut) if surface else np.float64(cut)


def links(x, radius, group, boxlo, boxhi, periodic, cut, surface=False, rsq=None):
    """bool [n, n]: i != j, both in the group, and rsq < cut cut -- or, with surface, rsq < s s with s = (ri + rj) + cut, each
    operation rounded once.  rsq is that of nbr_model.pair_rsq"""
    group = np.asarray(group, dtype=bool).reshape(-1)
    n = len(group)
    if rsq is None:
        rsq = nm.pair_rsq(x, boxlo, boxhi, periodic) if n else np.zeros((0, 0))
    cut = np.float64(cut)
    if surface:
        r = np.asarray(radius, dtype=np.float64).reshape(-1)
        s = (r[:, None] + r[None, :]) + cut
        near = rsq < s * s
    else:
        near = rsq < cut * cut
    return near & group[:, None] & group[None, :] & ~np.eye(n, dtype=bool)


def components(adj):
    """the connected components of a symmetric bool matrix: a list of index lists, by breadth-first search"""
    n = len(adj)
    seen = np.zeros(n, bool)
    out = []
    for s in range(n):
        if seen[s]:
            continue
        seen[s] = True
        comp, todo = [], deque([s])
        while todo:
            i = todo.popleft()
            comp.append(i)
            for j in np.nonzero(adj[i] & ~seen)[0]:
                seen[j] = True
                todo.append(int(j))
        out.append(comp)
    return out


def cluster_atom(x, radius, tags, group, boxlo, boxhi, periodic, cut, surface=False, rmax=None, rsq=None):
    """[n, 2] float64: the smallest tag of the atom's component and the number of atoms in it; 0 0 outside the group.  An
    isolated group atom has its own tag and 1.  rmax: the engine's largest radius (the largest of `radius` where None)"""
    tags = np.asarray(tags).reshape(-1)
    group = np.asarray(group, dtype=bool).reshape(-1)
    if rmax is None:
        rmax = float(np.max(radius)) if surface and len(tags) else 0.0
    nm.check_box(grid_cutoff(cut, surface, rmax), boxlo, boxhi, periodic)
    adj = links(x, radius, group, boxlo, boxhi, periodic, cut, surface, rsq)
    assert (adj == adj.T).all()
    out = np.zeros((len(tags), 2))
    for comp in components(adj):
        if not group[comp[0]]:
            continue
        out[comp, 0] = tags[comp].min()
        out[comp, 1] = len(comp)
    return out


def cluster_stats(ids, group):
    """[3] float64 over the atoms of `group` whose cluster ID is not 0: the distinct IDs, the most atoms under one ID, the atoms"""
    ids = np.asarray(ids).reshape(-1)
    sel = np.asarray(group, dtype=bool).reshape(-1) & (ids != 0)
    if not sel.any():
        return np.zeros(3)
    _, counts = np.unique(ids[sel], return_counts=True)
    return np.array([len(counts), counts.max(), sel.sum()], dtype=np.float64)
