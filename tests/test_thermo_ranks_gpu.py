"""Thermo output on a decomposed run (sf_lammps_open_world + `processors` + read_data), 2 and 4 ranks sharing the box's one
GPU over the stand-in wire (tests/c_abi/standin_rccl.cpp): only rank 0 writes; Step and Atoms are exact and every other
column is the single-domain run's to 1e-11 of the column's scale (the sums are combined over the ranks)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.rdzv import new_rendezvous
from tests.test_dump_ranks_gpu import _case, _script, _write_data
from tests.test_halo_gpu import _standin_rccl
from tests.test_thermo_gpu import _blocks

pytestmark = pytest.mark.gpu

STYLE = "thermo_style custom step atoms temp ke press pxx pyy pzz pxy pxz pyz fmax fnorm"
STEPS = (30, 30)


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
    # every rank names a file of its own: only rank 0's may appear
    for line in _script(bed, cfg, os.path.join(out, "bed.data"), grid) + [
            "log " + os.path.join(out, "log.rank%d" % rank), STYLE, "thermo 10"]:
        lmp.command(line)
    for n in STEPS:
        lmp.command("run %d" % n)
    vals = np.array([lmp.get_thermo(k) for k in STYLE.split()[2:]])
    np.save(os.path.join(out, "vals%d.npy" % rank), vals)
    dist.barrier()
    lmp.close()
    dist.destroy_process_group()


def _rows(path):
    return np.array([[float(t) for t in r.split()] for b in _blocks(path) for r in b[1]])


@pytest.mark.parametrize("world,grid", [(2, (2, 1, 1)), (4, (2, 1, 2))])
def test_thermo_on_ranks(tmp_path, world, grid):
    import torch.multiprocessing as mp
    from sedifoam_amd import Lammps
    bed, cfg = _case()
    data = str(tmp_path / "bed.data")
    _write_data(bed, data)
    ref = Lammps()
    for line in _script(bed, cfg, data, None) + ["log " + str(tmp_path / "ref.log"), STYLE, "thermo 10"]:
        ref.command(line)
    for n in STEPS:
        ref.command("run %d" % n)
    ref_vals = np.array([ref.get_thermo(k) for k in STYLE.split()[2:]])
    ref.close()
    lib = _standin_rccl(tmp_path)
    mp.spawn(_rank_worker, args=(world, new_rendezvous(), str(tmp_path), lib, grid), nprocs=world, join=True)
    assert os.path.exists(str(tmp_path / "log.rank0"))
    assert not any(os.path.exists(str(tmp_path / ("log.rank%d" % r))) for r in range(1, world))
    want, got = _rows(str(tmp_path / "ref.log")), _rows(str(tmp_path / "log.rank0"))
    assert got.shape == want.shape and list(got[:, 0]) == [0, 10, 20, 30, 30, 40, 50, 60]
    assert (got[:, :2] == want[:, :2]).all()   # Step, Atoms
    assert (got[:, 1] == len(bed["x"])).all()
    # the printed columns to print precision, the values behind them to 1e-11 of each column's scale
    for c in range(2, got.shape[1]):
        scale = max(np.max(np.abs(want[:, c])), 1e-300)
        assert np.max(np.abs(got[:, c] - want[:, c])) <= 1e-7 * scale, c
    # (the off-diagonal pressures are measured against the diagonal ones)
    scale = np.abs(ref_vals)
    scale[6:9] = np.max(np.abs(ref_vals[3:6]))
    for r in range(world):
        v = np.load(str(tmp_path / ("vals%d.npy" % r)))
        assert v.shape == ref_vals.shape
        assert np.all(np.abs(v - ref_vals) <= 1e-11 * np.maximum(scale, 1e-300)), (r, v, ref_vals)
