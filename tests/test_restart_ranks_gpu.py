"""Checkpoints on a decomposed run (sf_lammps_open_world + `processors`: the bricks of a `-parallel` run), 2 and 4 ranks
sharing one GPU over the stand-in wire.  Every rank reads the file and keeps the atoms of its brick; every rank packs its
atoms, rank 0 gathers, orders by tag and writes the one file.  (a) N ranks read F and write G: G == F byte for byte.
(b) N ranks read F and run m, a single domain does the same: the two files' arrays agree within 1e-9 (decomposition is
not bitwise: summation order), tags and contact pairs identical.  (c) a file written by 4 ranks is read by 2."""
import ctypes as C
import os

import numpy as np
import pytest

from sedifoam_amd import restart
from tests import dem_cases as dc
from tests.rdzv import new_rendezvous
from tests.test_dump_ranks_gpu import _case, _script, _write_data
from tests.test_halo_gpu import _standin_rccl

pytestmark = pytest.mark.gpu

K, M = 60, 40
TOL = 1e-9


def _resume_lines(bed, cfg, path, grid):
    lines = [l for l in dc.script_lines(bed, cfg) if not l.startswith(("boundary", "timestep"))]
    return lines[:1] + (["processors %d %d %d" % grid] if grid else []) + ["read_restart " + path] + lines[1:]


def _rank_worker(rank, world, port, out, rccl_lib, grid, src, names):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["SF_RCCL_LIB"] = rccl_lib
    import torch
    import torch.distributed as dist
    from sedifoam_amd import Lammps, lib
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=world)
    L = lib()
    ident = [None]
    if rank == 0:
        buf = C.create_string_buffer(128)
        assert L.sf_dem_comm_unique_id(buf) == 0
        ident[0] = buf.raw
    dist.broadcast_object_list(ident, src=0)
    h = C.c_void_p()
    assert L.sf_lammps_open_world(0, None, 0, rank, world, ident[0], C.byref(h)) == 0, L.sf_last_error()
    lmp = Lammps.__new__(Lammps)
    lmp.L, lmp.ptr = L, h
    bed, cfg = _case()
    for line in _resume_lines(bed, cfg, os.path.join(out, src), grid):
        lmp.command(line)
    nloc = lmp.get_local_n()
    lmp.command("write_restart " + os.path.join(out, names[0]))      # (a) / (c): without running
    if len(names) > 1:
        lmp.command("run %d" % M)                                     # (b)
        lmp.command("write_restart " + os.path.join(out, names[1]))
    np.savez(os.path.join(out, "%s.rank%d.npz" % (names[0], rank)), nloc=nloc)
    dist.barrier()
    lmp.close()
    dist.destroy_process_group()


def _close(a, b):
    assert np.array_equal(a["tag"], b["tag"]) and a["step"] == b["step"] == K + M
    assert np.array_equal(a["contact_count"], b["contact_count"])
    assert np.array_equal(a["contact_partner"], b["contact_partner"])
    err = {k: dc.rel_err(a[k], b[k]) for k in ("x", "v", "omega", "contact_shear")}
    assert [w["id"] for w in a["walls"]] == [w["id"] for w in b["walls"]]
    for k, (p, q) in enumerate(zip(a["walls"], b["walls"])):
        assert np.array_equal(p["tag"], q["tag"])
        if len(q["tag"]):
            err["wall%d" % k] = dc.rel_err(p["shear"], q["shear"])
    return err


def test_restart_on_ranks(tmp_path):
    import torch.multiprocessing as mp
    from sedifoam_amd import Lammps
    bed, cfg = _case()
    out = str(tmp_path)
    data = os.path.join(out, "bed.data")
    _write_data(bed, data)
    one = Lammps()
    for line in _script(bed, cfg, data, None):
        one.command(line)
    one.command("run %d" % K)
    assert one.info().nbuilds >= 2
    one.command("write_restart " + os.path.join(out, "F"))
    one.close()
    f = restart.read(os.path.join(out, "F"))
    assert sum(1 for s in f["contact_shear"] if np.any(s != 0.0)) >= 100 and len(f["walls"][0]["tag"]) >= 10
    ref = Lammps()
    for line in _resume_lines(bed, cfg, os.path.join(out, "F"), None):
        ref.command(line)
    ref.command("run %d" % M)
    ref.command("write_restart " + os.path.join(out, "H1"))
    ref.close()
    h1 = restart.read(os.path.join(out, "H1"))
    lib = _standin_rccl(tmp_path)
    F = open(os.path.join(out, "F"), "rb").read()
    for world, grid in ((2, (2, 1, 1)), (4, (2, 1, 2))):
        names = ("G%d" % world, "H%d" % world)
        mp.spawn(_rank_worker, args=(world, new_rendezvous(), out, lib, grid, "F", names), nprocs=world, join=True)
        nloc = [int(np.load(os.path.join(out, "%s.rank%d.npz" % (names[0], r)))["nloc"]) for r in range(world)]
        assert all(nloc) and sum(nloc) == len(f["tag"])                       # every brick keeps its atoms, each atom once
        assert open(os.path.join(out, names[0]), "rb").read() == F            # (a)
        err = _close(restart.read(os.path.join(out, names[1])), h1)           # (b)
        print("%d ranks against one domain after %d steps: %s" % (world, M, " ".join("%s=%.3e" % kv for kv in sorted(err.items()))))
        assert max(err.values()) <= TOL, err
    # (c) the file 4 ranks wrote, read by 2 and written back
    mp.spawn(_rank_worker, args=(2, new_rendezvous(), out, lib, (2, 1, 1), "H4", ("G4to2",)), nprocs=2, join=True)
    assert open(os.path.join(out, "G4to2"), "rb").read() == open(os.path.join(out, "H4"), "rb").read()
    assert sorted(n for n in os.listdir(out) if n[0] in "GH" and "rank" not in n) == ["G2", "G4", "G4to2", "H1", "H2", "H4"]
    assert not [n for n in os.listdir(out) if n.endswith(".tmp")]
