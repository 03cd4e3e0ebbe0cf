"""`dump custom` on a decomposed run (sf_lammps_open_world + `processors` + read_data: the bricks of a `-parallel` run),
2 and 4 ranks sharing the box's one GPU over the stand-in wire (tests/c_abi/standin_rccl.cpp).  One file: rank 0 writes
every rank's block in rank order, each tag once per frame; `%`: one file per rank whose union is that file; the values
are those of the single-domain run of the same script to print precision (decomposition is not bitwise)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import dem_cases as dc
from tests.rdzv import new_rendezvous
from tests.test_dump_gpu import frames
from tests.test_halo_gpu import _standin_rccl

pytestmark = pytest.mark.gpu

NCELLS = (8, 5, 8)
EVERY, STEPS = 20, (30, 30)


def _case():
    import tests.test_dem_gpu as T
    bed = T._bed(NCELLS, periodic=True, seed=41, vmax=0.5)
    cfg = dict(T.BASE, skin=0.05e-3)
    cfg["walls"] = T._walls(bed)
    return bed, cfg


def _write_data(bed, path):
    with open(path, "w") as f:
        f.write("dump ranks test\n\n%d atoms\n\n" % len(bed["x"]))
        for k, a in enumerate("xyz"):
            f.write("%.17g %.17g %slo %shi\n" % (bed["boxlo"][k], bed["boxhi"][k], a, a))
        f.write("\nAtoms\n\n")
        for i, x in enumerate(bed["x"]):
            f.write("%d 1 %.17g %.17g %.17g %.17g %.17g\n" % (i + 1, bed["diameter"][i], bed["density"][i], *x))


def _script(bed, cfg, data, grid):
    lines = dc.script_lines(bed, cfg)
    # the box comes from read_data: after atom_style / boundary (and `processors`), before the rest
    return lines[:2] + (["processors %d %d %d" % grid] if grid else []) + ["read_data " + data] + lines[2:]


def _dump_lines(out, world):
    cols = "id type x y z vx vy vz fx fy fz"
    return ["dump one all custom %d %s %s" % (EVERY, os.path.join(out, "one.dump"), cols),
            "dump per all custom %d %s %s" % (EVERY, os.path.join(out, "per.%.dump"), cols)]


def _rank_worker(rank, world, port, out, rccl_lib, grid):
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
    for line in _script(bed, cfg, os.path.join(out, "bed.data"), grid) + _dump_lines(out, world):
        lmp.command(line)
    try:
        lmp.command("dump_modify one sort id")
        refused = ""
    except Exception as ex:   # noqa: BLE001
        refused = str(ex)
    for n in STEPS:
        lmp.command("run %d" % n)
    li = lmp.get_local_info()
    np.savez(os.path.join(out, "rank%d.npz" % rank), tag=li["tag"], refused=np.array(refused))
    dist.barrier()
    lmp.close()
    dist.destroy_process_group()


def _rows_by_step(path):
    return {f[0]: f for f in frames(path)}


@pytest.mark.parametrize("world,grid", [(2, (2, 1, 1)), (4, (2, 1, 2))])
def test_dump_on_ranks_one_file_and_per_rank_files(tmp_path, world, grid):
    import torch.multiprocessing as mp
    bed, cfg = _case()
    data = str(tmp_path / "bed.data")
    _write_data(bed, data)
    # the single-domain run of the same script
    ref_dir = tmp_path / "ref"
    ref_dir.mkdir()
    from sedifoam_amd import Lammps
    ref = Lammps()
    for line in _script(bed, cfg, data, None) + _dump_lines(str(ref_dir), 1):
        ref.command(line)
    for n in STEPS:
        ref.command("run %d" % n)
    ref.close()
    want = _rows_by_step(str(ref_dir / "one.dump"))
    lib = _standin_rccl(tmp_path)
    mp.spawn(_rank_worker, args=(world, new_rendezvous(), str(tmp_path), lib, grid), nprocs=world, join=True)
    parts = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    assert all("sort id" in str(p["refused"]) for p in parts)   # one file on several ranks: no `sort id`
    assert all(len(p["tag"]) for p in parts)                     # every brick owns atoms
    got = _rows_by_step(str(tmp_path / "one.dump"))
    steps = list(range(0, sum(STEPS) + 1, EVERY))
    assert sorted(got) == sorted(want) == steps
    n = len(bed["x"])
    for s in steps:
        g, w = got[s], want[s]
        assert g[1] == n and g[2] == w[2]                        # count, box bounds and columns of the whole box
        ids = [int(r.split(b" ")[0]) for r in g[3]]
        assert sorted(ids) == list(range(1, n + 1))              # every tag exactly once
        vg = np.array([[float(t) for t in r.split()] for r in g[3]])
        vw = np.array([[float(t) for t in r.split()] for r in w[3]])
        vg = vg[np.argsort(vg[:, 0])]
        vw = vw[np.argsort(vw[:, 0])]
        assert (vg[:, :2] == vw[:, :2]).all()
        for c0, c1 in ((2, 5), (5, 8), (8, 11)):                 # x, v, f: print precision
            assert dc.rel_err(vg[:, c0:c1], vw[:, c0:c1]) <= 1e-5, (s, c0)
        # the `%` files of this step: one per rank, their union is the single file's frame
        per = [_rows_by_step(str(tmp_path / ("per.%d.dump" % r)))[s] for r in range(world)]
        assert sum(p[1] for p in per) == n
        assert sorted(b"".join(b"".join(p[3]) for p in per).splitlines()) == sorted(b"".join(g[3]).splitlines())
        # rank 0's block first (rank order): the single file's frame is the `%` files' frames one after the other
        assert b"".join(g[3]) == b"".join(b"".join(p[3]) for p in per)
    # the last frame is the state the run ended in: rank 0's atoms first, in its own order
    last = got[steps[-1]][3]
    n0 = len(parts[0]["tag"])
    assert [int(r.split(b" ")[0]) for r in last[:n0]] == [int(t) for t in parts[0]["tag"]]
