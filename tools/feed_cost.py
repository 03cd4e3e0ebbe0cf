"""Cost of the cloud's particle add / delete schedules on the headline bed, in one process, host
clock around synchronised calls:

  idle    one sub-cycle in which nobody leaves and no add is due: the mark launch and the flag read (sf_cloud_phase 7),
          against the host-driven route's look at the bed: get_local_info + the types, the box test in NumPy, no call
  event   one sub-cycle that clears about a thousand grains and adds one per cell of the top cell layer, against the
          host-driven route: the same lists from NumPy, Lammps.delete_particle and Lammps.create_particle

The host-driven route is what a shim had to do before the schedules were part of the library.  Both routes end in the same
rebuilds (one behind the clearing, one behind the add); those are in both `event` figures.

    python tools/feed_cost.py [--particles 1000000] [--settle 200] [--reps 5]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import enhancedCloud, synthetic
    from tests import feed_model as fm
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    lo, hi = bed["boxlo"], bed["boxhi"]
    d = float(np.max(bed["diameter"]))
    ytop = float(bed["x"][:, 1].max())
    mesh_n = np.array([max(2, int((hi[k] - lo[k]) / (2.7 * d))) for k in range(3)], np.int32)   # cells ~2.7 d wide
    dxm = (hi - lo) / mesh_n
    top_layer = (lo[0], hi[0], hi[1] - dxm[1], hi[1], lo[2], hi[2], 0.0, 0.0, 0.0)
    assert hi[1] - dxm[1] > ytop + d, "the top cell layer must be free of grains"
    side = 10.5 * d                                            # ~1 400 lattice sites x the share that is inside
    corner = (lo[0], lo[0] + side, ytop - 0.7 * side, ytop + d, lo[2], lo[2] + side, 0.0, 0.0, 0.0)
    nowhere = (-2.0, -1.0, -2.0, -1.0, -2.0, -1.0, 0.0, 0.0, 0.0)
    keys = dict(addParticle=1, deleteParticle=1, deleteBeforeAdd=1, randomPerturb=0.3 * d, addParticleBox=top_layer,
                addParticleInfo=(0.8 * d, 2000.0, 1), addParticleVelocity=(0.0, -1.0, 0.0), reduceNumberFactor=1)
    cdict = dict(dragModel="ErgunWenYu", subCycles=1)
    trans = dict(rhob=1000.0, nub=1.0e-6)
    deltaT = 50 * bench.KW["dt"]
    res = {"n": int(bed["n"]), "mesh": [int(k) for k in mesh_n]}

    def engine(feed):
        lmp = bench.build_engine(bed, script)
        lmp.setup()
        lmp.step(args.settle)
        cloud = enhancedCloud(lmp, lo, dxm, mesh_n, dict(cdict, **feed), trans, deltaT)
        lmp.sync()
        return lmp, cloud

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    # ---- idle ----
    lmp, cloud = engine(dict(keys, addParticleTimeStep=1.0e9, deleteParticleBox=corner, clearInitialBox=nowhere,
                             deleteParticle=1))
    cloud._phase(7)            # the first sub-cycle takes the corner's grains away; from then on nobody is inside
    res["idle_first_removed"] = cloud.feedInfo()["lastDelete"]
    ms = [timed(lambda: cloud._phase(7))[0] for _ in range(args.reps + 1)][1:]
    assert cloud.feedInfo()["lastDelete"] == 0
    res["idle_feed_ms"] = statistics.median(ms)
    res["idle_feed_ms_min_max"] = [min(ms), max(ms)]

    def host_lists(lmp, model):
        li = lmp.get_local_info()
        ii = lmp.get_initial_info()
        return model.sub_cycle_fast(li["x"], li["tag"], ii["type"])

    class Fast(fm.Schedule):
        """the model's sub-cycle with the box tests vectorised (region kind 1): what a host shim would write"""

        def box(self, b, x):
            return ((x[:, 0] - b[0]) * (x[:, 0] - b[1]) < fm.ROOTVSMALL) & ((x[:, 1] - b[2]) * (x[:, 1] - b[3]) < fm.ROOTVSMALL) & \
                ((x[:, 2] - b[4]) * (x[:, 2] - b[5]) < fm.ROOTVSMALL)

        def sub_cycle_fast(self, x, tag, typ):
            one = typ == 1
            add_due = self.time_to_add <= 0.0
            cleared = one & self.box(self.k["clearInitialBox"], x) if add_due else np.zeros(len(tag), bool)
            deleted = one & ~cleared & self.box(self.k["deleteParticleBox"], x)
            out = dict(clear=tag[cleared], delete=tag[deleted], add=None)
            if add_due:
                max_tag = int(tag[~cleared].max())
                nadd = len(self.cells)
                seed = len(tag) - int(cleared.sum()) + nadd - int(deleted.sum())
                c = self.centres[self.cells]
                g = fm.Lcg48(seed)
                u = np.array([g.next() for _ in range(3 * nadd)]).reshape(nadd, 3)
                out["add"] = dict(pos=c + float(self.k["randomPerturb"]) * (0.5 - u),
                                  tags=np.arange(max_tag + 1, max_tag + 1 + nadd, dtype=np.int32))
                self.time_to_add = self.step
            else:
                self.time_to_add -= self.deltaT
            return out

    centres = fm.cell_centres(lo, dxm, mesh_n)
    idle_keys = dict(keys, addParticleTimeStep=1.0e9, deleteParticleBox=corner, clearInitialBox=nowhere)
    model = Fast(idle_keys, centres, deltaT)
    ms = []
    for _ in range(args.reps + 1):
        t, w = timed(lambda: host_lists(lmp, model))
        assert len(w["delete"]) == 0
        ms.append(t)
    res["idle_host_ms"] = statistics.median(ms[1:])
    res["idle_host_ms_min_max"] = [min(ms[1:]), max(ms[1:])]
    cloud.close(); lmp.close()

    # ---- one event ----
    ev_keys = dict(keys, addParticleTimeStep=0.0, clearInitialBox=corner, deleteParticleBox=nowhere)
    lmp, cloud = engine(ev_keys)

    def fed():
        cloud._phase(7)
        lmp.sync()
    res["event_feed_ms"] = timed(fed)[0]
    info = cloud.feedInfo()
    res["event_cleared"], res["event_added"] = info["lastDeleteBeforeAdd"], info["lastAdd"]
    cloud.close(); lmp.close()
    lmp, cloud = engine({})
    model = Fast(ev_keys, centres, deltaT)

    def host():
        w = host_lists(lmp, model)
        lmp.delete_particle(w["clear"])
        lmp.create_particle(w["add"]["pos"], w["add"]["tags"], ev_keys["addParticleInfo"][0], ev_keys["addParticleInfo"][1], 1,
                            ev_keys["addParticleVelocity"])
        lmp.sync()
        return len(w["clear"]), len(w["add"]["tags"])
    res["event_host_ms"], (c, a) = timed(host)
    assert (c, a) == (res["event_cleared"], res["event_added"]), (c, a, res)
    print(res)


if __name__ == "__main__":
    main()
