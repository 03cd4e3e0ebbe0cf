"""Host-side mirror of the patched LAMMPS library interface the reference's OpenFOAM side binds
(interfaceToLammps/library.h:29-63).  Same names, argument meaning and buffers; the work happens in
libsedifoam_amd.so on the GPU."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SfError, check, dp, ip


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(dp if a.dtype == np.float64 else ip)


class Lammps:
    """`lammps_open` ... `lammps_close` (library.h:29-63)."""

    def __init__(self, comm=0, args=None):
        """args: LAMMPS command-line arguments after the program name, e.g. ["-log", "log.lammps", "-screen", "none"]"""
        self.L = _lib.lib()
        h = C.c_void_p()
        argv = [b"sedifoam_amd"] + [str(a).encode() for a in (args or [])]
        arr = (C.c_char_p * (len(argv) + 1))(*argv, None)
        check(self.L.sf_lammps_open(len(argv), C.cast(arr, C.c_void_p), comm, C.byref(h)))
        self.ptr = h

    def close(self):
        if self.ptr:
            check(self.L.sf_lammps_close(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- library.h:31-32 ----
    def command(self, line):
        err = self.L.sf_lammps_command(self.ptr, line.encode())
        if err is not None:
            raise SfError(err.decode())

    def commands(self, text):
        for line in text.splitlines():
            self.command(line)

    def file(self, path):
        check(self.L.sf_lammps_file(self.ptr, path.encode()))

    # ---- library.h:35-63 ----
    def get_global_n(self):
        return check(self.L.sf_lammps_get_global_n(self.ptr))

    def get_local_n(self):
        return check(self.L.sf_lammps_get_local_n(self.ptr))

    def get_initial_info(self):
        n = self.get_local_n()
        x = np.zeros((n, 3)); v = np.zeros((n, 3)); d = np.zeros(n); rho = np.zeros(n)
        tag = np.zeros(n, np.int32); cpu = np.zeros(n, np.int32); typ = np.zeros(n, np.int32)
        check(self.L.sf_lammps_get_initial_info(self.ptr, _p(x), _p(v), _p(d), _p(rho), _p(tag), _p(cpu), _p(typ)))
        return dict(x=x, v=v, diam=d, rho=rho, tag=tag, lmpCpuId=cpu, type=typ)

    def get_local_domain(self):
        d = np.zeros(6)
        check(self.L.sf_lammps_get_local_domain(self.ptr, _p(d)))
        return d

    def get_local_info(self):
        n = self.get_local_n()
        x = np.zeros((n, 3)); v = np.zeros((n, 3))
        foam = np.zeros(n, np.int32); cpu = np.zeros(n, np.int32); tag = np.zeros(n, np.int32)
        check(self.L.sf_lammps_get_local_info(self.ptr, _p(x), _p(v), _p(foam), _p(cpu), _p(tag)))
        return dict(x=x, v=v, foamCpuId=foam, lmpCpuId=cpu, tag=tag)

    def put_local_info(self, fdrag, tag, DuDt=None, foamCpuId=None):
        fdrag = _f64(fdrag).reshape(-1, 3)
        tag = _i32(tag)
        n = fdrag.shape[0]
        du = _f64(DuDt) if DuDt is not None else np.zeros((n, 3))
        cpu = _i32(foamCpuId) if foamCpuId is not None else np.zeros(n, np.int32)
        check(self.L.sf_lammps_put_local_info(self.ptr, n, _p(fdrag), _p(du), _p(cpu), _p(tag)))

    def step(self, n):
        check(self.L.sf_lammps_step(self.ptr, int(n)))

    def sync(self):
        """wait for the engine's stream and for the dump frames queued so far to be in their files"""
        check(self.L.sf_lammps_sync(self.ptr))

    def set_timestep(self, dt):
        check(self.L.sf_lammps_set_timestep(self.ptr, float(dt)))

    def get_timestep(self):
        return self.L.sf_lammps_get_timestep(self.ptr)

    def get_thermo(self, keyword):
        """a thermo keyword's value in the last thermo line written (lammps_get_thermo)"""
        v = C.c_double()
        check(self.L.sf_lammps_get_thermo(self.ptr, keyword.encode(), C.byref(v)))
        return v.value

    def thermo_launches(self):
        """kernel launches made for thermo lines so far"""
        n = C.c_longlong()
        check(self.L.sf_lammps_thermo_launches(self.ptr, C.byref(n)))
        return n.value

    def write_restart(self, path):
        """one checkpoint now (`write_restart FILE`; `*` = the current step); returns with the file complete"""
        check(self.L.sf_lammps_write_restart(self.ptr, str(path).encode()))

    def read_restart(self, path):
        """box, units, timestep, step counter, groups, atoms and their contact / wall history from a checkpoint; before a
        box exists, and pair_style / neighbor / the fixes are given again afterwards"""
        check(self.L.sf_lammps_read_restart(self.ptr, str(path).encode()))

    def restart_launches(self):
        """kernel launches made for checkpoints so far"""
        n = C.c_longlong()
        check(self.L.sf_lammps_restart_launches(self.ptr, C.byref(n)))
        return n.value

    def restart_cost(self, timing=True):
        """(GPU ms of the last checkpoint's pack, host ms until its pinned copy landed, host ms until its file was renamed);
        timing=True makes later checkpoints time their pack (which then waits for it)"""
        out = np.zeros(4)
        check(self.L.sf_lammps_restart_cost(self.ptr, int(timing), _p(out)))
        return tuple(out[:3])

    def contacts(self, group="all"):
        """the contact network now (what a `dump local` frame of a compute pair/local on `group` would hold, in its order):
        one row per touching pair of two atoms of the group, tag1 < tag2, evaluated from the current state with
        shearupdate = false.  dict of arrays: tag1, tag2, dist, force (signed normal force, repulsive > 0), f[n, 3] (the
        normal force on tag1), fs[n, 3] (the tangential force on tag1), fsmag.  Passive: the run goes on with the same bits"""
        g = group.encode()
        n = check(self.L.sf_lammps_get_contacts(self.ptr, g, 0, None, None, None))
        t1 = np.zeros(n, np.int32); t2 = np.zeros(n, np.int32); val = np.zeros((n, 9))
        if n:
            m = check(self.L.sf_lammps_get_contacts(self.ptr, g, n, _p(t1), _p(t2), _p(val)))
            assert m == n
        return dict(tag1=t1, tag2=t2, dist=val[:, 0].copy(), force=val[:, 1].copy(), f=val[:, 2:5].copy(),
                    fs=val[:, 5:8].copy(), fsmag=val[:, 8].copy())

    def contact_launches(self):
        """kernel launches made for contact rows so far"""
        n = C.c_longlong()
        check(self.L.sf_lammps_contact_launches(self.ptr, C.byref(n)))
        return n.value

    def contact_cost(self, group="all"):
        """(GPU ms of count + scan + rows, GPU ms of the text of every column, rows) of one evaluation now"""
        out = np.zeros(3)
        check(self.L.sf_lammps_contact_cost(self.ptr, group.encode(), _p(out)))
        return float(out[0]), float(out[1]), int(out[2])

    def compute_atom(self, cid):
        """the values of the per-atom compute `cid` (stress/atom: [n, 6] in the order xx yy zz xy xz yz; contact/atom,
        ke/atom, erotate/sphere/atom: [n]; property/atom: [n] for one attribute, [n, k] for several; cluster/atom: [n] the
        smallest tag of the atom's cluster, with size yes [n, 2] and the cluster's atom count behind it) now, sorted by tag like
        get_state(); atoms outside the compute's group read 0.
        What a `dump custom` column c_ID / c_ID[k] written at this moment holds.  Passive: the run goes on with the same bits"""
        cid = str(cid).encode()
        nc = C.c_int()
        n = check(self.L.sf_lammps_compute_atom(self.ptr, cid, 0, None, None, C.byref(nc)))
        tag = np.zeros(n, np.int32); val = np.zeros((n, max(nc.value, 1)))
        if n:
            m = check(self.L.sf_lammps_compute_atom(self.ptr, cid, n, _p(tag), _p(val), C.byref(nc)))
            assert m == n
        val = val[np.argsort(tag, kind="stable")]
        return val if nc.value > 1 else val[:, 0].copy()

    def compute_atom_launches(self):
        """kernel launches made for per-atom computes so far"""
        n = C.c_longlong()
        check(self.L.sf_lammps_compute_atom_launches(self.ptr, C.byref(n)))
        return n.value

    def compute_atom_cost(self, cid):
        """GPU ms of one fresh evaluation of the per-atom compute `cid` now"""
        ms = C.c_double()
        check(self.L.sf_lammps_compute_atom_cost(self.ptr, str(cid).encode(), C.byref(ms)))
        return ms.value

    def ave_chunk(self, fid):
        """the latest output of `fix fid group ave/chunk ...`: dict(step, coord[nchunk, ndim] (the centres of the layers),
        count[nchunk] (Ncount), values[nchunk, nvalues], names (the value words as typed)), chunk 1 first -- what the
        fix's file holds for that step.  An error before the first output"""
        fid = str(fid).encode()
        step = C.c_longlong(); nd = C.c_int(); nv = C.c_int()
        n = check(self.L.sf_lammps_ave_chunk(self.ptr, fid, 0, C.byref(step), C.byref(nd), C.byref(nv), None, None, None))
        coord = np.zeros((n, nd.value)); count = np.zeros(n); val = np.zeros((n, nv.value))
        m = check(self.L.sf_lammps_ave_chunk(self.ptr, fid, n, C.byref(step), C.byref(nd), C.byref(nv), _p(coord), _p(count),
                                             _p(val)))
        assert m == n
        nb = check(self.L.sf_lammps_ave_chunk_names(self.ptr, fid, 0, None))
        buf = C.create_string_buffer(nb)
        check(self.L.sf_lammps_ave_chunk_names(self.ptr, fid, nb, buf))
        return dict(step=step.value, coord=coord, count=count, values=val, names=buf.value.decode().split())

    def ave_chunk_launches(self):
        """kernel launches made for chunk/atom computes and fix ave/chunk so far"""
        n = C.c_longlong()
        check(self.L.sf_lammps_ave_chunk_launches(self.ptr, C.byref(n)))
        return n.value

    def ave_chunk_cost(self, fid):
        """GPU ms of (assign, sort + segment offsets, sums + fold) of one sample of fix ave/chunk `fid` now; passive"""
        out = np.zeros(3)
        check(self.L.sf_lammps_ave_chunk_cost(self.ptr, str(fid).encode(), _p(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def compute_global(self, cid):
        """the values of the global compute `cid` (compute reduce, ke, erotate/sphere, com; cluster/stats: the number of
        clusters, the largest one's atoms, the atoms in clusters) on the state as it stands: a float64 array, length 1 for a
        scalar; not normalised.  What a fix ave/time sample or a thermo column c_ID / c_ID[k] taken at
        this moment holds.  Passive: the run goes on with the same bits"""
        cid = str(cid).encode()
        vec = C.c_int()
        n = check(self.L.sf_lammps_compute_global(self.ptr, cid, 0, None, C.byref(vec)))
        val = np.zeros(n)
        m = check(self.L.sf_lammps_compute_global(self.ptr, cid, n, _p(val), C.byref(vec)))
        assert m == n
        return val

    def ave_time(self, fid):
        """the latest output of `fix fid group ave/time ...`: dict(step, values[nvalues], names (the value words as typed))
        -- what the last line of the fix's file holds.  An error before the first output"""
        fid = str(fid).encode()
        step = C.c_longlong()
        n = check(self.L.sf_lammps_ave_time(self.ptr, fid, 0, C.byref(step), None))
        val = np.zeros(n)
        m = check(self.L.sf_lammps_ave_time(self.ptr, fid, n, C.byref(step), _p(val)))
        assert m == n
        nb = check(self.L.sf_lammps_ave_time_names(self.ptr, fid, 0, None))
        buf = C.create_string_buffer(nb)
        check(self.L.sf_lammps_ave_time_names(self.ptr, fid, nb, buf))
        rows = check(self.L.sf_lammps_ave_time_rows(self.ptr, fid))
        if rows > 0:   # mode vector: values[nrows, nvalues]
            val = val.reshape(rows, n // rows)
        return dict(step=step.value, values=val, names=buf.value.decode().split())

    def compute_array(self, cid):
        """the global array of `compute cid group rdf Nbin [itype jtype ...] cutoff Rc` on the positions as they stand:
        float64 [Nbin, 1 + 2 npairs] -- the bin centre, then g(r) and the running coordination number of each pair.  What a
        fix ave/time mode vector sample taken at this moment holds.  A per-chunk compute (property/chunk, com/chunk, vcm/chunk,
        gyration/chunk) gives float64 [Nchunk, ncol], row m - 1 chunk m: [Nchunk, 1] for one column, (0, ncol) without chunks.
        Passive: the run goes on with the same bits"""
        cid = str(cid).encode()
        nc = C.c_int()
        n = check(self.L.sf_lammps_compute_array(self.ptr, cid, 0, None, C.byref(nc)))
        val = np.zeros(n)
        m = check(self.L.sf_lammps_compute_array(self.ptr, cid, n, _p(val), C.byref(nc)))
        assert m == n
        return val.reshape(n // nc.value, nc.value)

    def rdf_counts(self, cid):
        """the raw counts of compute rdf `cid`: dict(counts int64 [npairs, Nbin] ordered pairs per bin, icount, jcount,
        duplicates int64 [npairs])"""
        cid = str(cid).encode()
        npairs = C.c_int()
        n = check(self.L.sf_lammps_rdf_counts(self.ptr, cid, 0, None, None, C.byref(npairs)))
        counts = np.zeros(n, np.int64)
        per = np.zeros(3 * npairs.value, np.int64)
        ll = C.POINTER(C.c_longlong)
        m = check(self.L.sf_lammps_rdf_counts(self.ptr, cid, n, counts.ctypes.data_as(ll), per.ctypes.data_as(ll), C.byref(npairs)))
        assert m == n
        per = per.reshape(npairs.value, 3)
        return dict(counts=counts.reshape(npairs.value, n // npairs.value), icount=per[:, 0].copy(), jcount=per[:, 1].copy(),
                    duplicates=per[:, 2].copy())

    def nbr_launches(self):
        """dict(grid_builds, launches, host_copies): cutoff grids built, kernel launches made and device-to-host copies made
        for compute rdf, coord/atom and cluster/atom so far (cluster/atom: one 4-byte copy per verify round)"""
        g = C.c_longlong(); n = C.c_longlong(); h = C.c_longlong()
        check(self.L.sf_lammps_nbr_launches(self.ptr, C.byref(g), C.byref(n), C.byref(h)))
        return dict(grid_builds=g.value, launches=n.value, host_copies=h.value)

    def nbr_cost(self, cid):
        """GPU ms of (one fresh grid build, one walk) of compute rdf, coord/atom or cluster/atom `cid` now; the walk of a
        cluster/atom is everything after the grid, the waits for the flag of its verify rounds included"""
        g = C.c_double(); w = C.c_double()
        check(self.L.sf_lammps_nbr_cost(self.ptr, str(cid).encode(), C.byref(g), C.byref(w)))
        return g.value, w.value

    def cluster_rounds(self, cid):
        """the verify rounds of the last evaluation of compute cluster/atom `cid`: 1 unless a verify launch had to hook a
        pair the hook launch left apart; 0 before the first evaluation"""
        r = C.c_int()
        check(self.L.sf_lammps_cluster_rounds(self.ptr, str(cid).encode(), C.byref(r)))
        return r.value

    def chunk_info(self, cid):
        """dict(nchunk, ids, launches, host_copies) of `compute cid group chunk/atom c_ID ...` on the state as it stands: ids
        int32 [nchunk], the original IDs under compress yes and 1 .. nchunk otherwise; launches and host_copies: the kernel
        launches and the device-to-host copies (4 bytes each: Nchunk) that the evaluations of this compute and of the per-chunk
        computes over it have made so far"""
        cid = str(cid).encode()
        la = C.c_longlong(); hc = C.c_longlong()
        n = check(self.L.sf_lammps_chunk_info(self.ptr, cid, 0, None, C.byref(la), C.byref(hc)))
        ids = np.zeros(n, np.int32)
        m = check(self.L.sf_lammps_chunk_info(self.ptr, cid, n, ids.ctypes.data_as(C.POINTER(C.c_int)), C.byref(la), C.byref(hc)))
        assert m == n
        return dict(nchunk=int(n), ids=ids, launches=la.value, host_copies=hc.value)

    def chunk_cost(self, cid):
        """GPU ms of one evaluation now of chunk/atom compute `cid` (over c_ID) and of every per-chunk compute over it; the
        compute behind c_ID is evaluated before the clock starts"""
        ms = C.c_double()
        check(self.L.sf_lammps_chunk_cost(self.ptr, str(cid).encode(), C.byref(ms)))
        return ms.value

    def global_launches(self):
        """dict(launches, host_copies): kernel launches made for global computes and fix ave/time so far, and the
        device-to-host copies made for them (outputs, thermo lines and queries; none at a sample that is not an output)"""
        n = C.c_longlong(); h = C.c_longlong()
        check(self.L.sf_lammps_global_launches(self.ptr, C.byref(n), C.byref(h)))
        return dict(launches=n.value, host_copies=h.value)

    def global_cost(self, cid):
        """GPU ms of one fresh evaluation of the global compute `cid` now"""
        ms = C.c_double()
        check(self.L.sf_lammps_global_cost(self.ptr, str(cid).encode(), C.byref(ms)))
        return ms.value

    def images(self):
        """ix iy iz of the owned atoms, (n, 3) int32 in the atom order of get_local_info(): how many box lengths the
        periodic wrap has taken each atom back by, so that x + images() * (boxhi - boxlo) is the unwrapped position (the
        xu yu zu of compute property/atom).  One rank, no fix rigid/nve; on an engine filled through
        create_atoms the counting starts with the first call or keyword that needs it, which must come before the first
        run"""
        n = self.get_local_n()
        out = np.zeros((n, 3), np.int32)
        check(self.L.sf_lammps_get_image(self.ptr, _p(out)))
        return out

    def region_match(self, rid, points):
        """bool per point of `points` (n, 3): does it match region `rid` (its side applied)?  Evaluated on the GPU by the
        device function the group kernels call; the points need not lie in the box"""
        p = _f64(points).reshape(-1, 3)
        out = np.zeros(p.shape[0], np.int32)
        check(self.L.sf_lammps_region_match(self.ptr, str(rid).encode(), p.shape[0], _p(p), _p(out)))
        return out.astype(bool)

    def group_mask(self, name):
        """bool per owned atom, in the atom order of get_local_info(): is it in group `name`?"""
        out = np.zeros(self.get_local_n(), np.int32)
        check(self.L.sf_lammps_group_mask(self.ptr, str(name).encode(), _p(out)))
        return out.astype(bool)

    def group_count(self, name):
        """the owned atoms of group `name`: of a dynamic group the device counter of the last launch that evaluated or counted
        it; of any other group, and of a dynamic group no launch has counted since its definition, a count made now"""
        return check(self.L.sf_lammps_group_count(self.ptr, str(name).encode()))

    def region_launches(self):
        """launches of the region match kernels so far (one per step at which dynamic groups are due, however many)"""
        n = C.c_longlong()
        check(self.L.sf_lammps_region_launches(self.ptr, C.byref(n)))
        return n.value

    def region_cost(self, name=None):
        """GPU ms of one update of the dynamic group `name` (None: of all dynamic groups in their one launch) now; passive"""
        ms = C.c_double()
        check(self.L.sf_lammps_region_cost(self.ptr, str(name).encode() if name else None, C.byref(ms)))
        return ms.value

    def ave_histo(self, fid):
        """the latest output of `fix fid group ave/histo ...`: dict(step, nbins, total, missing, min, max, coord[nbins],
        count[nbins], frac[nbins] (count / total, 0 when total is 0)) -- what the last block of the fix's file holds.  An
        error before the first output"""
        fid = str(fid).encode()
        step = C.c_longlong()
        stats = np.zeros(4)
        n = check(self.L.sf_lammps_ave_histo(self.ptr, fid, 0, C.byref(step), _p(stats), None, None))
        coord = np.zeros(n); count = np.zeros(n)
        m = check(self.L.sf_lammps_ave_histo(self.ptr, fid, n, C.byref(step), _p(stats), _p(coord), _p(count)))
        assert m == n
        total = float(stats[0])
        frac = count / total if total > 0.0 else np.zeros(n)
        return dict(step=step.value, nbins=n, total=total, missing=float(stats[1]), min=float(stats[2]), max=float(stats[3]),
                    coord=coord, count=count, frac=frac)

    def ave_histo_launches(self):
        """dict(launches, host_copies): binning launches made for fix ave/histo so far, and the device-to-host copies (one
        per output; none at a sample that is not an output)"""
        n = C.c_longlong(); h = C.c_longlong()
        check(self.L.sf_lammps_ave_histo_launches(self.ptr, C.byref(n), C.byref(h)))
        return dict(launches=n.value, host_copies=h.value)

    def ave_histo_cost(self, fid):
        """GPU ms of the binning of one sample of fix ave/histo `fid` now; passive"""
        ms = C.c_double()
        check(self.L.sf_lammps_ave_histo_cost(self.ptr, str(fid).encode(), C.byref(ms)))
        return ms.value

    def set_molecule(self, tags, mol):
        """molecule IDs of the atoms with these tags (what `read_data FILE fix ID NULL Molecules` reads from a file)"""
        t, m = _i32(tags), _i32(mol)
        assert t.shape == m.shape
        check(self.L.sf_lammps_set_molecule(self.ptr, t.shape[0], _p(t), _p(m)))

    def rigid_bodies(self):
        """the bodies of fix rigid/nve, ordered by the smallest tag they hold: natoms, masstotal, xcm, vcm, fcm, torque,
        angmom, omega, inertia (principal moments), quat (w x y z)"""
        nb = check(self.L.sf_lammps_get_rigid(self.ptr, 0, *([None] * 10)))
        out = dict(natoms=np.zeros(nb, np.int32), masstotal=np.zeros(nb), xcm=np.zeros((nb, 3)), vcm=np.zeros((nb, 3)),
                   fcm=np.zeros((nb, 3)), torque=np.zeros((nb, 3)), angmom=np.zeros((nb, 3)), omega=np.zeros((nb, 3)),
                   inertia=np.zeros((nb, 3)), quat=np.zeros((nb, 4)))
        if nb:
            check(self.L.sf_lammps_get_rigid(self.ptr, nb, *[_p(out[k]) for k in (
                "natoms", "masstotal", "xcm", "vcm", "fcm", "torque", "angmom", "omega", "inertia", "quat")]))
        return out

    def create_particle(self, position, tag, diameter, rho, type_, vel):
        position = _f64(position).reshape(-1, 3)
        t = _f64(tag)
        check(self.L.sf_lammps_create_particle(self.ptr, position.shape[0], _p(position), _p(t), diameter, rho,
                                               type_, _p(_f64(vel))))

    def delete_particle(self, tags):
        t = _i32(tags)
        check(self.L.sf_lammps_delete_particle(self.ptr, _p(t), t.shape[0]))

    # ---- engine extras (sf_dem_*) ----
    def create_atoms(self, x, diameter, density, v=None, omega=None, tag=None, type_=None):
        x = _f64(x).reshape(-1, 3)
        n = x.shape[0]
        check(self.L.sf_dem_create_atoms(
            self.ptr, n, _p(x), _p(_f64(v).reshape(-1, 3)) if v is not None else None,
            _p(_f64(omega).reshape(-1, 3)) if omega is not None else None, _p(_f64(diameter)),
            _p(_f64(density)), _p(_i32(tag)) if tag is not None else None,
            _p(_i32(type_)) if type_ is not None else None))

    def set_box(self, lo, hi):
        check(self.L.sf_dem_set_box(self.ptr, _p(_f64(lo)), _p(_f64(hi))))

    def setup(self):
        check(self.L.sf_dem_setup(self.ptr))

    def info(self):
        out = _lib.DemInfo()
        check(self.L.sf_dem_get_info(self.ptr, C.byref(out)))
        return out

    def lane_reuse_fraction(self):
        """Of the (atom, slot) pairs of the current list with a next lane (waves of 64 consecutive atoms) and a next slot:
        the fraction whose next slot names the root the next lane's slot names (what SF_LANE_REUSE serves from registers)."""
        out = C.c_double()
        check(self.L.sf_dem_lane_reuse_fraction(self.ptr, C.byref(out)))
        return out.value

    def device_view(self):
        out = _lib.DemDeviceView()
        check(self.L.sf_dem_device_view_get(self.ptr, C.byref(out)))
        return out

    def set_profiling(self, on=True):
        check(self.L.sf_dem_set_profiling(self.ptr, int(on)))

    def get_profile(self):
        """(launches, summed kernel milliseconds) of the fused sub-step kernel, from HIP events."""
        n = C.c_longlong(); ms = C.c_double()
        check(self.L.sf_dem_get_profile(self.ptr, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def get_rebuild_profile(self):
        """(neighbour rebuilds inside runs while profiling was on, their summed host-clock milliseconds)"""
        n = C.c_longlong(); ms = C.c_double()
        check(self.L.sf_dem_get_rebuild_profile(self.ptr, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def get_state(self):
        """x, v, omega, f, torque of the owned atoms sorted by tag."""
        n = self.get_local_n()
        li = self.get_local_info()
        f = np.zeros((n, 3)); t = np.zeros((n, 3)); w = np.zeros((n, 3)); tag = np.zeros(n, np.int32)
        check(self.L.sf_dem_get_forces(self.ptr, _p(f), _p(t), _p(w), _p(tag)))
        assert (tag == li["tag"]).all()
        o = np.argsort(tag, kind="stable")
        return dict(x=li["x"][o], v=li["v"][o], omega=w[o], f=f[o], torque=t[o], tag=tag[o])

    def history(self):
        """{(tag_i, tag_j): shear[3]} for touching pairs, tag_i < tag_j."""
        cap = max(int(self.info().npairs_full), 1)
        ti = np.zeros(cap, np.int32); tj = np.zeros(cap, np.int32); sh = np.zeros((cap, 3))
        n = check(self.L.sf_dem_get_history(self.ptr, cap, _p(ti), _p(tj), _p(sh)))
        return {(int(a), int(b)): s.copy() for a, b, s in zip(ti[:n], tj[:n], sh[:n])}

    def neighbors(self):
        """every word of the full list of the owned atoms, in no particular order: an (n, 5) int array of
        tag_i, tag_j, sx, sy, sz (which periodic image of j; 0 0 0 = j itself) and the flags (bit 0: the pair touches,
        bit 1: this side stores the pair's history).  Single domain only; changes nothing."""
        cap = max(int(self.info().npairs_full), 1)
        ti = np.zeros(cap, np.int32); tj = np.zeros(cap, np.int32)
        im = np.zeros((cap, 3), np.int32); fl = np.zeros(cap, np.int32)
        n = check(self.L.sf_dem_get_neighbors(self.ptr, cap, _p(ti), _p(tj), _p(im), _p(fl)))
        assert n <= cap, (n, cap)
        return np.column_stack([ti[:n], tj[:n], im[:n]]).astype(np.int64), fl[:n].copy()

    def build_positions(self):
        """x, tag: the positions the current list was built from (what the skin/2 check measures from), engine order"""
        n = self.get_local_n()
        x = np.zeros((n, 3)); tag = np.zeros(n, np.int32)
        check(self.L.sf_dem_get_build_positions(self.ptr, _p(x), _p(tag)))
        return x, tag

    def wall_shear(self, w):
        n = self.get_local_n()
        sh = np.zeros((n, 3))
        check(self.L.sf_dem_get_wall_shear(self.ptr, w, _p(sh)))
        tag = self.get_local_info()["tag"]
        return sh[np.argsort(tag, kind="stable")]
