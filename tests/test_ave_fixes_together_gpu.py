"""One fix ave/chunk, one fix ave/time and one fix ave/histo side by side (csrc/sf_ave_fix.hip: the one ID space of the three
kinds, `unfix`, the cuts of a run and the order of the samples within a step).  The code under test is host code, so the bed is
the 108-grain bed of tests/test_global_gpu.py and nothing is compared with a model: each fix writes, next to the other two, the
bytes it writes alone in a fresh engine over the same pieces of a run (the other test files hold each kind to its model)."""
import pytest

from sedifoam_amd import SfError
from tests import dem_cases as dc
from tests.test_ave_chunk_gpu import Y1
from tests.test_contacts_gpu import _small
from tests.test_global_gpu import _third

pytestmark = pytest.mark.gpu

# (the fix ave/histo bins the global vector c_w, and the fix ave/time averages c_w[2]: on the steps where both sample, the
# compute is in the one plan of global computes once)
FIXES = {"p": "fix p all ave/chunk 2 3 10 cy vx density/mass c_k",
         "t": "fix t all ave/time 2 3 10 c_r c_w[2] c_K start 20",
         "h": "fix h all ave/histo 5 2 10 -2.0 2.0 8 c_w mode vector beyond end ave window 2"}
PIECES = (7, 13, 30)


def _engine():
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    for line in ("compute cy all chunk/atom " + Y1, "compute k all ke/atom", "compute r all reduce sum vx",
                 "compute w all reduce sum vx vy vz", "compute K all ke"):
        lmp.command(line)
    return lmp


def _files(tmp, which):
    """the bytes of the files of the fixes `which` after run 7, run 13, run 30, unfix t, run 20"""
    tmp.mkdir()
    lmp = _engine()
    for fid in which:
        lmp.command("%s file %s" % (FIXES[fid], tmp / (fid + ".txt")))
    for n in PIECES:
        lmp.command("run %d" % n)
    if "t" in which:
        lmp.command("unfix t")
    lmp.command("run 20")
    if "h" in which:
        assert lmp.ave_histo("h")["step"] == 70 and lmp.ave_histo("h")["total"] == 2 * 2 * 3   # (a window of two outputs)
    lmp.close()
    return {fid: open(tmp / (fid + ".txt"), "rb").read() for fid in which}


def _output_steps(text, ntitles, nrows):
    lines = text.decode().splitlines()[ntitles:]
    return [int(ln.split()[0]) for ln in lines[::1 + nrows]]


def test_each_file_is_what_its_fix_writes_alone(tmp_path):
    together = _files(tmp_path / "all", "pth")
    nchunk = int(together["p"].decode().splitlines()[3].split()[1])
    assert nchunk > 1
    assert _output_steps(together["p"], 3, nchunk) == [10, 20, 30, 40, 50, 60, 70]
    assert _output_steps(together["t"], 2, 0) == [20, 30, 40, 50]   # (start 20; removed at step 50)
    assert _output_steps(together["h"], 3, 8) == [10, 20, 30, 40, 50, 60, 70]
    for fid in "pth":
        alone = _files(tmp_path / fid, fid)
        assert together[fid] == alone[fid], fid


def test_one_id_space_unfix_and_uncompute(tmp_path):
    lmp = _engine()
    for fid in "pth":
        lmp.command(FIXES[fid])
    for taken in "pth":
        for kind in "pth":
            line = FIXES[kind].split()
            with pytest.raises(SfError, match="fix %s %s: this fix ID is in use" % (line[3], taken)):
                lmp.command(" ".join(["fix", taken] + line[2:]))
    for cid, style in (("cy", "ave/chunk"), ("k", "ave/chunk"), ("r", "ave/time"), ("K", "ave/time"), ("w", "ave/time")):
        with pytest.raises(SfError, match="uncompute %s: a fix %s still uses this compute \\(unfix it first\\)" % (cid, style)):
            lmp.command("uncompute " + cid)
    lmp.command("unfix t")
    with pytest.raises(SfError, match="uncompute w: a fix ave/histo still uses this compute \\(unfix it first\\)"):
        lmp.command("uncompute w")
    # every ID goes on to another kind: t is free, then p, then h
    for fid, kind in (("t", "h"), ("p", "t"), ("h", "p")):
        if fid != "t":
            lmp.command("unfix " + fid)
        lmp.command(" ".join(["fix", fid] + FIXES[kind].split()[2:]))
    with pytest.raises(SfError, match="unfix nope: only a fix ave/chunk can be removed"):
        lmp.command("unfix nope")
    lmp.command("run 20")
    assert lmp.ave_histo("t")["step"] == 20 and lmp.ave_time("p")["step"] == 20 and lmp.ave_chunk("h")["step"] == 20
    for fid, style in (("t", "ave/time"), ("p", "ave/chunk"), ("h", "ave/histo")):
        with pytest.raises(SfError, match="Could not find fix %s ID %s" % (style, fid)):
            getattr(lmp, style.replace("/", "_"))(fid)
    for fid in "pth":
        lmp.command("unfix " + fid)
    for cid in ("r", "w", "K", "k", "cy"):
        lmp.command("uncompute " + cid)
    lmp.command("run 5")   # (nothing is left that cuts the run)
    lmp.close()
