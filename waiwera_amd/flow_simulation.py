"""Host-side mirror of the reference's flow_simulation_type (src/flow_simulation.F90), i.e. the
concrete ode_type (src/ode.F90:39-108) whose hot loops now run as HIP kernels.

Method names, argument order and the `err` convention follow the reference's type-bound
procedures (lhs, rhs, pre_eval, pre_iteration, pre_timestep, pre_retry_timestep,
post_linesearch, setup_jacobian); the SNES/KSP slots the reference fills with PETSc objects
(src/timestepper.F90:1552-1836) are the residual / jacobian / ksp_solve / newton_step methods.
Vectors are numpy arrays (host) or torch tensors (device): both are passed by address.
"""
import ctypes as C

import numpy as np

from . import lib as _lib
from .lib import LIB, WaiError


def box_aggregates(ijk, boxes):
    """aggregate of every cell of a structured mesh for set_pc_coarse: the cells' index range along every axis cut into
    boxes[a] equal parts (the last ones shorter where it does not divide), numbered x-major; ijk: (n, 3) cell indices"""
    ijk = np.asarray(ijk, dtype=np.int64)
    boxes = tuple(int(b) for b in boxes)
    if len(boxes) != 3 or min(boxes) < 1:
        raise ValueError("boxes: three positive counts (nx, ny, nz)")
    lo, hi = ijk.min(axis=0), ijk.max(axis=0) + 1
    if any(boxes[a] > hi[a] - lo[a] for a in range(3)):
        raise ValueError("boxes %r: more boxes than cells along an axis of extent %r" % (boxes, tuple((hi - lo).tolist())))
    idx = [(ijk[:, a] - lo[a]) * boxes[a] // (hi[a] - lo[a]) for a in range(3)]
    return ((idx[0] * boxes[1] + idx[1]) * boxes[2] + idx[2]).astype(np.int32)


class FlowSimulation:
    def __init__(self, mesh, eos="we", opts=None, device=0, temperature=20.0,
                 relperm=("linear", [0.0, 1.0, 0.0, 1.0]), capillary=("zero", []), thermo="iapws",
                 permeability_modifier=None, thermo_extrapolate=False):
        self.mesh = mesh
        self.eos_name = eos
        self._keep = dict(
            face_cells=_lib._i32(mesh.face_cells), face_geom=_lib._f64(mesh.face_geom),
            cell_geom=_lib._f64(mesh.cell_geom), rock=_lib._f64(mesh.rock),
            sub_ptr=_lib._i32(mesh.sub_ptr) if mesh.sub_ptr is not None else None)
        k = self._keep
        md = _lib.MeshDesc()
        md.n_owned, md.n_halo, md.n_bc, md.n_faces = mesh.n_owned, mesh.n_halo, mesh.n_bc, mesh.n_faces
        md.face_cells = k["face_cells"].ctypes.data_as(_lib.pi)
        md.face_geom = k["face_geom"].ctypes.data_as(_lib.pd)
        md.cell_geom = k["cell_geom"].ctypes.data_as(_lib.pd)
        md.rock = k["rock"].ctypes.data_as(_lib.pd)
        if k["sub_ptr"] is not None:
            md.n_sub = k["sub_ptr"].size - 1
            md.sub_ptr = k["sub_ptr"].ctypes.data_as(_lib.pi)
        self.eos_desc = _lib.eos_desc(eos, temperature, relperm, capillary, thermo=thermo,
                                      permeability_modifier=permeability_modifier)
        self.opts = opts or _lib.default_opts()
        h = C.c_void_p()
        rc = LIB.wai_ctx_create(C.byref(md), C.byref(self.eos_desc), C.byref(self.opts), device, C.byref(h))
        self.h = h
        if rc != 0:
            msg = LIB.wai_last_error(h).decode() if h else "?"
            raise WaiError("wai_ctx_create failed (%d): %s" % (rc, msg))
        # "table" curves (before the boundary fluid is evaluated in wai_set_bc)
        for spec, keys in ((relperm, ((0, "liquid", [[0, 0], [1, 1]]), (1, "vapour", [[0, 0], [1, 1]]))),
                           (capillary, ((2, "pressure", [[0, 0], [1, 0]]),))):
            if spec[0] == "table":
                for which, key, default in keys:
                    xy = _lib._f64(spec[1].get(key, default))
                    self._chk(LIB.wai_set_curve_table(h, which, _lib.INTERP[spec[1].get("interpolation", "linear")],
                                                      len(xy), xy.ctypes.data_as(_lib.pd)), "set_curve_table")
        if thermo_extrapolate:      # before the boundary fluid is evaluated, like the curve tables
            self.set_thermo_extrapolate(True)
        self.num_primary_variables = LIB.wai_block_size(h)
        self.fluid_dof = LIB.wai_num_fluid_dof(h)
        self.n_owned, self.n_prim, self.n_local = mesh.n_owned, mesh.n_prim, mesh.n_local
        self.num_dof = self.n_owned * self.num_primary_variables
        self.num_tracers, self.auxiliary = 0, False
        self.tracer_solve_mode = "per_tracer"
        self.sub_pc = "ilu"
        self.time = 0.0
        self.rank, self.world = 0, 1      # comm_init: this rank in the library's communicator
        if mesh.n_bc:
            bp, br = _lib._f64(mesh.bc_primary), _lib._i32(mesh.bc_region)
            self._chk(LIB.wai_set_bc(h, bp.ctypes.data_as(_lib.pd), br.ctypes.data_as(_lib.pi)), "set_bc")
        if mesh.n_src:
            sc, sr = _lib._i32(mesh.src_cell), _lib._f64(mesh.src_rate)
            se, sk = _lib._f64(mesh.src_enthalpy), _lib._i32(mesh.src_component)
            self._chk(LIB.wai_set_sources(h, sc.size, sc.ctypes.data_as(_lib.pi), sr.ctypes.data_as(_lib.pd),
                                          se.ctypes.data_as(_lib.pd), sk.ctypes.data_as(_lib.pi)), "set_sources")
        if mesh.nbr_ranks is not None and len(mesh.nbr_ranks):
            nr, sp = _lib._i32(mesh.nbr_ranks), _lib._i32(mesh.send_ptr)
            si, rp = _lib._i32(mesh.send_idx), _lib._i32(mesh.recv_ptr)
            self._chk(LIB.wai_set_halo(h, nr.size, nr.ctypes.data_as(_lib.pi), sp.ctypes.data_as(_lib.pi),
                                       si.ctypes.data_as(_lib.pi), rp.ctypes.data_as(_lib.pi)), "set_halo")

    def set_thermo_extrapolate(self, on):
        """"thermodynamics.extrapolate" (wai_set_thermo_extrapolate): region 1 (liquid water) is evaluated up to 360 deg C
        instead of 350, the formulas as they are.  The boundary cells' fluid is evaluated when the object is made: a mesh
        with boundary cells hotter than 350 deg C needs the constructor's thermo_extrapolate=True"""
        self._chk(LIB.wai_set_thermo_extrapolate(self.h, 1 if on else 0), "set_thermo_extrapolate")

    def thermo_extrapolate(self):
        on = C.c_int(0)
        self._chk(LIB.wai_get_thermo_extrapolate(self.h, C.byref(on)), "thermo_extrapolate")
        return bool(on.value)

    def set_source_production_component(self, components):
        """"source.production_component" (wai_set_source_production_component), one integer per source or None: a
        producing source with c > 0 puts its whole rate into component c (c = the number of primary variables: heat alone,
        no enthalpy formed); c <= 0 keeps production on the source's `component` as before"""
        if components is None:
            self._chk(LIB.wai_set_source_production_component(self.h, None), "set_source_production_component")
            return
        pc = _lib._i32(components)
        if pc.size != self.mesh.n_src:
            raise ValueError("one production component per source")
        self._chk(LIB.wai_set_source_production_component(self.h, pc.ctypes.data_as(_lib.pi) if pc.size else None),
                  "set_source_production_component")

    def update_rock(self, field, cells, values):
        """rock controls: one field of the rock record (0..2 permeability, 3 wet, 4 dry conductivity, 5 porosity,
        6 density, 7 specific heat) on the listed local cells, before a try"""
        ci, v = _lib._i32(cells), _lib._f64(np.broadcast_to(np.asarray(values, dtype=np.float64), np.shape(cells)))
        self._chk(LIB.wai_update_rock(self.h, int(field), ci.size, ci.ctypes.data_as(_lib.pi), v.ctypes.data_as(_lib.pd)), "update_rock")
        self.mesh.rock[ci, field] = v

    def set_source_rates(self, rate=None, enthalpy=None):
        """new rates / enthalpies of the sources in force (what table controls do before a try)"""
        r = _lib._f64(rate) if rate is not None else None
        e = _lib._f64(enthalpy) if enthalpy is not None else None
        for a in (r, e):
            if a is not None and a.size != self.mesh.n_src:
                raise ValueError("one value per source")
        self._chk(LIB.wai_update_sources(self.h, r.ctypes.data_as(_lib.pd) if r is not None else None,
                                         e.ctypes.data_as(_lib.pd) if e is not None else None), "update_sources")

    def set_source_controls(self, records):
        """state-dependent controls, one dict per source (waiwera_amd.lib.source_controls) or None"""
        if records is None:
            self._chk(LIB.wai_set_source_controls(self.h, None), "set_source_controls")
            return
        if len(records) != self.mesh.n_src:
            raise ValueError("one control record per source")
        self._chk(LIB.wai_set_source_controls(self.h, _lib.source_controls(records)), "set_source_controls")

    def set_source_network(self, spec):
        """groups and reinjectors (include/waiwera_hip.h, wai_set_source_network).  spec: dict(rate_specified,
        enthalpy_specified per source; groups [dict(inputs=[(kind, index)], scaling 0 | 1, limits=[(type, limit)])];
        reinjectors [dict(input=(kind, index), outputs=[dict(flow 1 | 2, out=(kind, index), rate, proportion,
        enthalpy)], overflow=(kind, index))]); kinds 0 none, 1 source, 2 group, 3 reinjector"""
        g, r = spec["groups"], spec["reinjectors"]
        self._net_keep, args = _lib.network_arrays(spec)
        self._chk(LIB.wai_set_source_network(self.h, *args), "set_source_network")
        self._net_sizes = (len(g), len(r))

    def set_source_global_index(self, n_global, global_index):
        """a source network across ranks: the global index of each of this rank's sources (the description given
        to set_source_network is then numbered globally, the same on every rank)"""
        gi = _lib._i32(global_index)
        self._gidx_keep = gi
        self._chk(LIB.wai_set_source_global_index(self.h, int(n_global), gi.ctypes.data_as(_lib.pi)), "set_source_global_index")

    def source_network(self):
        """(groups (n, 6): rate, enthalpy, water_rate, water_enthalpy, steam_rate, steam_enthalpy;
        reinjectors (n, 8): output water / steam rate, overflow rate, enthalpy, water rate, water enthalpy, steam
        rate, steam enthalpy) after the last residual evaluation"""
        ng, nr = getattr(self, "_net_sizes", (0, 0))
        G, R = np.zeros((max(ng, 1), 6)), np.zeros((max(nr, 1), 8))
        self._chk(LIB.wai_get_source_network(self.h, G.ctypes.data_as(_lib.pd), R.ctypes.data_as(_lib.pd)), "get_source_network")
        return G[:ng], R[:nr]

    def set_network_pass(self, where):
        """where the source network's pass runs (wai_set_network_pass): "host" (default: rates to the host, the network walked
        there, factors back -- two stream waits per pass) or "device" (one launch walks it in LDS; the coupling build then
        waits once per Jacobian).  The same bits either way.  Before or after set_source_network"""
        if where not in _lib.NETWORK_PASS:
            raise ValueError("network pass %r: one of %s" % (where, sorted(_lib.NETWORK_PASS)))
        self._chk(LIB.wai_set_network_pass(self.h, _lib.NETWORK_PASS[where]), "set_network_pass")

    def network_pass(self):
        """(requested, in_force): the setting, and what runs -- "host" on several ranks, for a network too large for a
        workgroup's LDS, and without a network"""
        r, f = C.c_int(0), C.c_int(0)
        self._chk(LIB.wai_get_network_pass(self.h, C.byref(r), C.byref(f)), "network_pass")
        name = {v: k for k, v in _lib.NETWORK_PASS.items()}
        return name[r.value], name[f.value]

    def set_network_walk(self, how):
        """how the device pass walks groups and reinjectors (wai_set_network_walk): "lane" (default: one lane of the wave, a
        network of at most 64 KB of LDS) or "wave" (the 64 lanes gather every sum's terms and one chains them in input order;
        dynamic LDS up to 160 KiB).  The same bits either way.  Before or after set_source_network"""
        if how not in _lib.NETWORK_WALK:
            raise ValueError("network walk %r: one of %s" % (how, sorted(_lib.NETWORK_WALK)))
        self._chk(LIB.wai_set_network_walk(self.h, _lib.NETWORK_WALK[how]), "set_network_walk")

    def network_walk(self):
        """(requested, in_force): the setting, and what runs -- "wave" where the device pass is in force (network_pass) and
        the wave schedule accepts the network, "lane" otherwise"""
        r, f = C.c_int(0), C.c_int(0)
        self._chk(LIB.wai_get_network_walk(self.h, C.byref(r), C.byref(f)), "network_walk")
        name = {v: k for k, v in _lib.NETWORK_WALK.items()}
        return name[r.value], name[f.value]

    def network_stats(self):
        """(passes, host_waits): network passes so far, and the stream waits passes and coupling builds issued"""
        p, w = C.c_longlong(0), C.c_longlong(0)
        self._chk(LIB.wai_test_network_stats(self.h, C.byref(p), C.byref(w)), "network_stats")
        return p.value, w.value

    def set_coupling_build(self, how):
        """how wai_jacobian builds the network's coupling blocks (wai_set_coupling_build): "columns" (default: one column at a
        time on the global state) or "batched" (all columns at once on private scratch, five launches whatever the number of
        network cells).  The same bits either way.  Before or after set_source_network"""
        if how not in _lib.COUPLING_BUILD:
            raise ValueError("coupling build %r: one of %s" % (how, sorted(_lib.COUPLING_BUILD)))
        self._chk(LIB.wai_set_coupling_build(self.h, _lib.COUPLING_BUILD[how]), "set_coupling_build")

    def coupling_build(self):
        """(requested, in_force): the setting, and what runs -- "batched" where the device pass is in force (network_pass)
        and the couplings are on, "columns" otherwise"""
        r, f = C.c_int(0), C.c_int(0)
        self._chk(LIB.wai_get_coupling_build(self.h, C.byref(r), C.byref(f)), "coupling_build")
        name = {v: k for k, v in _lib.COUPLING_BUILD.items()}
        return name[r.value], name[f.value]

    def coupling_build_stats(self):
        """(launches, columns, chunks) of the last coupling build (wai_test_coupling_build_stats)"""
        a, b, c = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        self._chk(LIB.wai_test_coupling_build_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "coupling_build_stats")
        return a.value, b.value, c.value

    def set_network_couplings(self, on=True, in_preconditioner=True):
        """the network's Jacobian blocks (flow_simulation_modify_jacobian, flow_simulation.F90:3023-3084) on / off;
        in_preconditioner: also inside the factor's pattern, as PETSc factors the widened matrix (default), or in the
        operator only"""
        self._chk(LIB.wai_set_network_couplings(self.h, (2 if in_preconditioner else 1) if on else 0), "set_network_couplings")

    def network_couplings(self):
        """(cells (m,), E (ml, m, bs, bs)): d R(cell i) / d y(cell j) through the network pass, of the last
        wai_jacobian (wai_get_network_couplings); m = 0 without a network or when E vanishes.  One rank: ml = m.
        A network on several ranks: the columns are the network's cells of all ranks ordered by (owner, cell), the
        rows this rank's own (cells >= 0, in that order); another rank's cell reads -1 - owner"""
        m = C.c_int(0)
        self._chk(LIB.wai_get_network_couplings(self.h, C.byref(m), None, None), "get_network_couplings")
        bs = self.num_primary_variables
        cells = np.zeros(m.value, dtype=np.int32)
        if not m.value:
            return cells, np.zeros((0, 0, bs, bs))
        self._chk(LIB.wai_get_network_couplings(self.h, C.byref(m), cells.ctypes.data_as(_lib.pi), None), "get_network_couplings")
        E = np.zeros((int((cells >= 0).sum()), m.value, bs, bs))
        if E.size:
            self._chk(LIB.wai_get_network_couplings(self.h, C.byref(m), None, E.ctypes.data_as(_lib.pd)), "get_network_couplings")
        return cells, E

    def separator_enthalpies(self, pressure):
        hf, hg = C.c_double(0.0), C.c_double(0.0)
        self._chk(LIB.wai_separator_enthalpies(self.h, pressure, C.byref(hf), C.byref(hg)), "separator_enthalpies")
        return hf.value, hg.value

    def source_rates(self, collective=False):
        """(rate, enthalpy) of every source on the current fluid.  collective: a source network across ranks -- the call
        runs the network pass, which gathers all ranks' sources, so a rank WITHOUT sources makes it too"""
        r, e = np.zeros(self.mesh.n_src), np.zeros(self.mesh.n_src)
        if self.mesh.n_src or collective:
            self._chk(LIB.wai_get_source_rates(self.h, r.ctypes.data_as(_lib.pd), e.ctypes.data_as(_lib.pd)), "get_source_rates")
        return r, e

    # ------------------------------------------------------------------------------------------
    def _chk(self, rc, what):
        if rc < 0:
            raise WaiError("%s failed (%d): %s" % (what, rc, LIB.wai_last_error(self.h).decode()))
        return rc

    def destroy(self):
        if self.h:
            LIB.wai_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def set_opts(self, **kw):
        for k, v in kw.items():
            if k == "ksp_type" and isinstance(v, str):
                v = _lib.KSP[v]
            if k == "pc_type" and isinstance(v, str):
                v = _lib.PC[v]
            setattr(self.opts, k, v)
        self._chk(LIB.wai_set_opts(self.h, C.byref(self.opts)), "set_opts")

    def comm_init(self, rank, nranks, unique_id):
        self._chk(LIB.wai_comm_init(self.h, rank, nranks, unique_id), "comm_init")
        self.rank, self.world = int(rank), int(nranks)

    def comm_size(self):
        return LIB.wai_comm_size(self.h)

    def comm_stats(self):
        a, e = C.c_longlong(0), C.c_longlong(0)
        LIB.wai_comm_stats(self.h, C.byref(a), C.byref(e))
        return a.value, e.value

    def gather_stats(self):
        """gathers to a root enqueued on this rank so far (wai_gather_stats)"""
        g = C.c_longlong(0)
        LIB.wai_gather_stats(self.h, C.byref(g))
        return g.value

    @staticmethod
    def _gather_out(out, n_global, ncomp, is_root):
        """the root's result array: the caller's (numpy or torch, n_global x ncomp doubles) or a NaN-filled one -- a place
        nobody sends stays NaN"""
        if not is_root:
            return None
        if out is None:
            out = np.full((int(n_global), int(ncomp)), np.nan)
        return out

    def gather_rows(self, local, index, n_global, root=0, out=None):
        """wai_gather_rows (collective): this rank's rows local (n_local, ncomp) -- numpy or a torch device tensor -- to
        out[index] on `root`; returns the (n_global, ncomp) array there (out, or a new one filled with NaN), None on the
        other ranks"""
        if hasattr(local, "data_ptr"):
            loc, n_local = local, int(local.shape[0])
            ncomp = int(local.numel() // max(n_local, 1)) if n_local else int(local.shape[1])
        else:
            loc = _lib._f64(local)
            loc = loc[:, None] if loc.ndim == 1 else loc
            if loc.ndim != 2 or loc.shape[1] < 1:
                raise ValueError("local: (n_local, ncomp) rows")
            n_local, ncomp = loc.shape
        idx = _lib._i32(index)
        if idx.size != n_local:
            raise ValueError("one place per row: %d rows, %d places" % (n_local, idx.size))
        res = self._gather_out(out, n_global, ncomp, self.rank == root)
        self._chk(LIB.wai_gather_rows(self.h, int(root), int(ncomp), _lib.ptr(loc) if n_local else None, n_local,
                                      idx.ctypes.data if n_local else None, int(n_global), _lib.ptr(res)), "gather_rows")
        return res

    def gather_fluid(self, fields, index, n_global, root=0, which=0, out=None):
        """wai_gather_fluid (collective): columns `fields` of the fluid record of this rank's owned cells, packed on the
        device, to out[index] on `root`; returns the (n_global, len(fields)) array there, None elsewhere"""
        fl, idx = _lib._i32(fields), _lib._i32(index)
        if idx.size != self.n_owned:
            raise ValueError("one place per owned cell")
        res = self._gather_out(out, n_global, fl.size, self.rank == root)
        self._chk(LIB.wai_gather_fluid(self.h, int(root), int(which), fl.size, fl.ctypes.data_as(_lib.pi), idx.ctypes.data,
                                       int(n_global), _lib.ptr(res)), "gather_fluid")
        return res

    def mute_comm(self, on):
        """timing probe: collectives return without calling RCCL (every rank together)"""
        self._chk(LIB.wai_bench_mute_comm(self.h, 1 if on else 0), "bench_mute_comm")

    def drop_stream_wait(self, which):
        """fault injection (tests): 1 the face bricks' launch does not wait for the halo exchange, 0 off"""
        self._chk(LIB.wai_test_drop_stream_wait(self.h, int(which)), "test_drop_stream_wait")

    def halo_size(self, dof=None):
        """(bytes this rank sends per halo exchange of a dof-per-cell vector, neighbours)"""
        b, n = C.c_longlong(0), C.c_int(0)
        LIB.wai_halo_size(self.h, self.num_primary_variables if dof is None else dof, C.byref(b), C.byref(n))
        return b.value, n.value

    def launch_stats(self):
        """(kernels launched, copies enqueued) by the linear-solver helpers so far"""
        a, e = C.c_longlong(0), C.c_longlong(0)
        LIB.wai_launch_stats(self.h, C.byref(a), C.byref(e))
        return a.value, e.value

    def pc_kernel_name(self, composed=False):
        """kernel (or path) of a preconditioned-operator application; composed: its form with the operand R - alpha V
        made inside the launch (the second fused launch of a BiCGStab iteration where bcgs_composed() says so)"""
        name = LIB.wai_pc_kernel_name(self.h).decode()
        if composed:
            name = name[:-1] + ",composed>" if name.endswith(">") else name + " (composed operand)"
        return name

    def bcgs_composed(self):
        return LIB.wai_bcgs_composed(self.h) == 1

    def set_regions(self, region):
        r = _lib._i32(region)
        assert r.size == self.n_prim
        self._chk(LIB.wai_set_regions(self.h, r.ctypes.data_as(_lib.pi)), "set_regions")

    def regions(self):
        r = np.zeros(self.n_prim, dtype=np.int32)
        self._chk(LIB.wai_get_regions(self.h, r.ctypes.data_as(_lib.pi)), "get_regions")
        return r

    def fluid(self, which=0):
        """Fluid vector in the reference's AoS layout (n_local, fluid_dof)."""
        out = np.zeros((self.n_local, self.fluid_dof))
        self._chk(LIB.wai_get_fluid(self.h, which, out.ctypes.data), "get_fluid")
        return out

    def fluxes(self):
        """(n_faces, np + nmob): component and phase fluxes per unit area, cell 1 -> cell 2 (the reference's flux vector)"""
        nf = LIB.wai_num_flux_dof(self.h)
        out = np.zeros((self.mesh.n_faces, nf))
        self._chk(LIB.wai_get_fluxes(self.h, out.ctypes.data), "get_fluxes")
        return out

    def source_separated(self, collective=False):
        """(n_sources, 4): water_rate, water_enthalpy, steam_rate, steam_enthalpy behind each source's separator
        (collective: as source_rates)"""
        out = np.zeros((max(self.mesh.n_src, 1), 4))
        if self.mesh.n_src or collective:
            self._chk(LIB.wai_get_source_separated(self.h, out.ctypes.data_as(_lib.pd)), "get_source_separated")
        return out[: self.mesh.n_src]

    def scale(self, primary, region):
        """eos%scale (src/eos.F90:186-197): unscaled primaries (n, np) -> scaled y."""
        sc = np.ones((9, self.num_primary_variables))
        ps, ts = self.eos_desc.pressure_scale, self.eos_desc.temperature_scale
        for r in (1, 2, 4, 5, 6, 8):     # 5, 6, 8: eos wse regions with halite (src/eos_wse.F90:155-165)
            sc[r, 0] = ps
            if self.num_primary_variables > 1:
                sc[r, 1] = ts if r not in (4, 8) else 1.0
        prim = np.asarray(primary, dtype=np.float64)
        out = prim / sc[np.asarray(region)]
        if self.eos_name in ("wce", "wae") and self.eos_desc.partial_pressure_scale <= 0:
            out[..., 2] = prim[..., 2] / prim[..., 0]  # adaptive Pg / P (eos_wge.F90:639-655)
        if self.eos_name in ("wsce", "wsae"):           # 4th primary: Pg / P, or Pg over its scale
            ppsc = self.eos_desc.partial_pressure_scale
            out[..., 3] = prim[..., 3] / (prim[..., 0] if ppsc <= 0 else ppsc)
        return out

    # ---- ode_type hooks ------------------------------------------------------------------------
    def pre_timestep(self):
        return self._chk(LIB.wai_pre_timestep(self.h), "pre_timestep")

    def pre_try_timestep(self, t):
        return 0  # rock controls (flow_simulation.F90:2039-2089) are out of scope

    def pre_retry_timestep(self):
        return self._chk(LIB.wai_pre_retry_timestep(self.h), "pre_retry_timestep")

    def post_timestep(self):
        return 0

    def pre_iteration(self, y=None):
        return self._chk(LIB.wai_pre_iteration(self.h), "pre_iteration")

    def pre_eval(self, t, y, perturbed_columns=None):
        if perturbed_columns is not None and len(perturbed_columns):
            raise WaiError("coloured perturbation is replaced by wai_jacobian")
        return self._chk(LIB.wai_pre_eval(self.h, t, _lib.ptr(y)), "pre_eval")

    pre_solve = pre_eval

    def lhs(self, t, interval, y, lhs):
        return self._chk(LIB.wai_lhs(self.h, t, _lib.ptr(y), _lib.ptr(lhs)), "lhs")

    def rhs(self, t, interval, y, rhs):
        return self._chk(LIB.wai_rhs(self.h, t, _lib.ptr(y), _lib.ptr(rhs)), "rhs")

    def post_linesearch(self, y_old, search, y):
        cs, cy = C.c_int(0), C.c_int(0)
        err = self._chk(LIB.wai_post_linesearch(self.h, _lib.ptr(y_old), _lib.ptr(search), _lib.ptr(y),
                                                C.byref(cs), C.byref(cy)), "post_linesearch")
        return bool(cs.value), bool(cy.value), err

    def setup_jacobian(self):
        nnzb = LIB.wai_jacobian_nnzb(self.h)
        rp = np.zeros(self.n_owned + 1, dtype=np.int32)
        ci = np.zeros(nnzb, dtype=np.int32)
        self._chk(LIB.wai_jacobian_pattern(self.h, rp.ctypes.data_as(_lib.pi), ci.ctypes.data_as(_lib.pi)),
                  "jacobian_pattern")
        return rp, ci

    # ---- SNES / KSP slots ------------------------------------------------------------------------
    def set_residual_form(self, method="beuler", ratio=0.0, lhs_last2=None):
        """Residual the SNES slots evaluate: the method's `residual` pointer
        (src/timestepper.F90:1484-1500); bdf2 needs ratio = dt / last dt and the lhs two steps back."""
        p = _lib.ptr(lhs_last2) if lhs_last2 is not None else None
        return self._chk(LIB.wai_set_residual_form(self.h, _lib.METHOD_KIND[method], ratio, p),
                         "set_residual_form")

    def set_timestep_method(self, method="beuler"):
        """Method `timestep` integrates with; the library then keeps the BDF2 history."""
        return self._chk(LIB.wai_set_timestep_method(self.h, _lib.METHOD_KIND[method]),
                         "set_timestep_method")

    def residual(self, t, dt, y, lhs_old, f):
        return self._chk(LIB.wai_residual(self.h, t, dt, _lib.ptr(y), _lib.ptr(lhs_old), _lib.ptr(f)), "residual")

    def jacobian(self, t, dt, y, lhs_old):
        return self._chk(LIB.wai_jacobian(self.h, t, dt, _lib.ptr(y), _lib.ptr(lhs_old)), "jacobian")

    def jacobian_values(self):
        nnzb, bs = LIB.wai_jacobian_nnzb(self.h), self.num_primary_variables
        v = np.zeros(nnzb * bs * bs)
        self._chk(LIB.wai_jacobian_get_values(self.h, v.ctypes.data), "jacobian_get_values")
        return v

    def set_jacobian_values(self, val):
        v = _lib._f64(val) if isinstance(val, np.ndarray) else val
        self._chk(LIB.wai_jacobian_set_values(self.h, _lib.ptr(v)), "jacobian_set_values")

    def spmv(self, x, y):
        return self._chk(LIB.wai_spmv(self.h, _lib.ptr(x), _lib.ptr(y)), "spmv")

    def pc_setup(self):
        return self._chk(LIB.wai_pc_setup(self.h), "pc_setup")

    def pc_apply(self, r, z):
        return self._chk(LIB.wai_pc_apply(self.h, _lib.ptr(r), _lib.ptr(z)), "pc_apply")

    def pc_operator(self, x, x2=None, alpha=0.0, dot_mode=0, aux=None, spmv=True, split=False, fin_phase=-2, scal_in=None):
        """one preconditioned-operator application as the Krylov drivers issue it (tests): z = B^-1 A (x - alpha x2)
        (spmv) or B^-1 x, with dot_mode's inner products finished in the launch (fin_phase >= -1: and that phase's
        BiCGStab scalars derived) or by k_finalize (-2); (z, the 16 device scalars after)"""
        xi = _lib._f64(x)
        x2i = _lib._f64(x2) if x2 is not None else None
        ai = _lib._f64(aux) if aux is not None else None
        s_in = _lib._f64(np.zeros(16) if scal_in is None else scal_in)
        assert xi.size == self.num_dof and s_in.size == 16
        z, s_out = np.zeros(self.num_dof), np.zeros(16)
        self._chk(LIB.wai_test_pc_operator(self.h, 1 if spmv else 0, _lib.ptr(xi), _lib.ptr(x2i), float(alpha), int(dot_mode),
                                           _lib.ptr(ai), 1 if split else 0, int(fin_phase), s_in.ctypes.data_as(_lib.pd),
                                           _lib.ptr(z), s_out.ctypes.data_as(_lib.pd)), "test_pc_operator")
        return z, s_out

    def pc_axpy_capable(self):
        """can the fused launch form its operand x - alpha x2 itself (pc_operator's x2)?"""
        return LIB.wai_pc_axpy_capable(self.h) == 1

    def partial_count(self):
        """partial sums per reduction slot the last preconditioner application left (wai_test_partial_count)"""
        return self._chk(LIB.wai_test_partial_count(self.h), "test_partial_count")

    def desc_templates(self):
        """(distinct descriptor templates, bricks, template rows) of the brick schedule k_pc_park reads on its 16-bit column
        indices (wai_test_desc_templates); (0, bricks, 0) when the schedule has none"""
        nb, nr = C.c_int(0), C.c_int(0)
        nt = self._chk(LIB.wai_test_desc_templates(self.h, C.byref(nb), C.byref(nr)), "test_desc_templates")
        return nt, nb.value, nr.value

    def pack_groups(self, which=0):
        """(groups, bricks that share a workgroup, table [groups][8][4]) of the packed k_pc_park launch over list `which` -- 0
        all subdomains, 1 interior bricks, 2 face bricks (wai_test_pack_groups); (0, 0, empty) where every brick has its own
        workgroup"""
        shared = C.c_int(0)
        ng = self._chk(LIB.wai_test_pack_groups(self.h, which, C.byref(shared), None, 0), "test_pack_groups")
        table = np.zeros(ng * 32, dtype=np.int32)
        if ng:
            self._chk(LIB.wai_test_pack_groups(self.h, which, C.byref(shared), table.ctypes.data_as(C.POINTER(C.c_int)), table.size),
                      "test_pack_groups")
        return ng, shared.value, table.reshape(ng, 8, 4)

    KV_OPS = ("dot", "dots", "waxpy", "bcgs_p", "bcgs_s", "bcgs_xr", "bcgs_xrp", "bcgs_xrp_derive", "scalars", "mdot",
              "maxpy_norm", "scale_to", "update_x")
    KV_VECS = ("X", "R", "RP", "P", "V", "S", "T")

    def krylov_vec(self, op, n, vecs, scal, variant=0, k=0, ld=0, basis=None, coef=None, alpha=0.0):
        """one vector / reduction step of the Krylov drivers through their own launchers (tests; wai_test_krylov_vec):
        vecs (7, len) in KV_VECS order, scal the 128 device scalars, basis (k + 1) * ld doubles.  Nothing passed in is
        changed; (vecs, basis, scal, post) after, post = [(R,R), breakdown code] as posted to the host or NaNs"""
        v = np.array(vecs, dtype=np.float64, order="C")
        s = np.array(scal, dtype=np.float64)
        assert v.ndim == 2 and v.shape[0] == len(self.KV_VECS) and s.shape == (128,)
        b = np.array(basis, dtype=np.float64).ravel() if basis is not None else None
        assert b is None or b.size == (k + 1) * ld
        cf = _lib._f64(coef) if coef is not None else None
        assert cf is None or cf.size >= k
        post = np.full(2, np.nan)
        P = lambda a: a.ctypes.data_as(_lib.pd) if a is not None else None   # noqa: E731
        self._chk(LIB.wai_test_krylov_vec(self.h, self.KV_OPS.index(op), int(variant), int(n), int(k), int(ld), v.shape[1],
                                          float(alpha), P(v), P(b), P(cf), P(s), P(post)), "test_krylov_vec")
        return v, b, s, post

    def ksp_solve(self, b, x):
        its, reason, rn = C.c_int(0), C.c_int(0), C.c_double(0)
        self._chk(LIB.wai_ksp_solve(self.h, _lib.ptr(b), _lib.ptr(x), C.byref(its), C.byref(reason),
                                    C.byref(rn)), "ksp_solve")
        return its.value, reason.value, rn.value

    def max_scaled(self, v, scale, tol):
        val, idx = C.c_double(0), C.c_int(0)
        self._chk(LIB.wai_max_scaled(self.h, _lib.ptr(v), _lib.ptr(scale), tol, C.byref(val), C.byref(idx)),
                  "max_scaled")
        return val.value, idx.value

    def newton_step(self, t, dt, it, y, lhs_old, f):
        k, r, m = C.c_int(0), C.c_int(0), C.c_double(0)
        self._chk(LIB.wai_newton_step(self.h, t, dt, it, _lib.ptr(y), _lib.ptr(lhs_old), _lib.ptr(f),
                                      C.byref(k), C.byref(r), C.byref(m)), "newton_step")
        return r.value, k.value, m.value

    def timestep(self, t, dt, y):
        n, k, r = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(LIB.wai_timestep(self.h, t, dt, _lib.ptr(y), C.byref(n), C.byref(k), C.byref(r)), "timestep")
        return r.value, n.value, k.value

    def set_tracer_injection(self, injection):
        """[n_sources][nt] tracer injection rates (tracer table controls set them per step interval)"""
        self._chk(LIB.wai_set_tracer_injection(self.h, _lib.ptr(_lib._f64(np.asarray(injection, dtype=np.float64)))),
                  "set_tracer_injection")

    # ---- tracers: the auxiliary linear problem (ode_type aux_lhs / aux_rhs / aux_pre_solve) ------
    def set_tracers(self, phase, decay=None, activation=None, diffusion=None, bc=None, injection=None):
        """Passive tracers (src/tracer.F90:30-40): 0-based phase index, decay constant, activation
        energy, diffusion coefficient per tracer; bc [n_bc][nt] Dirichlet mass fractions, injection
        [n_sources][nt] tracer injection rates."""
        nt = len(phase)
        ph = np.ascontiguousarray(phase, dtype=np.int32)

        def arr(a):
            return _lib._f64(np.zeros(nt) if a is None else np.asarray(a, dtype=np.float64))
        dc, ac, df = arr(decay), arr(activation), arr(diffusion)
        self._chk(LIB.wai_set_tracers(self.h, nt, ph.ctypes.data_as(C.POINTER(C.c_int)),
                                      dc.ctypes.data_as(C.POINTER(C.c_double)),
                                      ac.ctypes.data_as(C.POINTER(C.c_double)),
                                      df.ctypes.data_as(C.POINTER(C.c_double))), "set_tracers")
        self.num_tracers = nt
        self.auxiliary = nt > 0
        if bc is not None:
            self._chk(LIB.wai_set_tracer_bc(self.h, _lib.ptr(_lib._f64(np.asarray(bc, dtype=np.float64)))), "set_tracer_bc")
        if injection is not None:
            self._chk(LIB.wai_set_tracer_injection(self.h, _lib.ptr(_lib._f64(np.asarray(injection, dtype=np.float64)))),
                      "set_tracer_injection")

    def set_tracer_solve_mode(self, mode):
        """"per_tracer" (default): one scalar Krylov solve per tracer; "coupled": all tracers in one solve on the
        [cell][tracer] vector, as the reference's auxiliary KSPSolve (block Jacobi ILU(0) or no preconditioner; others
        are refused by aux_solve)"""
        self._chk(LIB.wai_set_tracer_solve_mode(self.h, _lib.TRACER_SOLVE[mode]), "set_tracer_solve_mode")
        self.tracer_solve_mode = mode

    def set_sub_pc(self, sub):
        """sub-preconditioner of pc_type bjacobi / asm: "ilu" (default, ILU(ilu_levels)) or "lu", the exact LU of every
        (overlapped) block, factored and applied on the device; ignored under pc_type none and lu"""
        self._chk(LIB.wai_set_sub_pc(self.h, _lib.SUB_PC[sub]), "set_sub_pc")
        self.sub_pc = sub

    def set_pc_ordering(self, ordering):
        """elimination order of the flow system's block-Jacobi ILU(0) (wai_set_pc_ordering): "natural" (default, the
        reference's) or "multicolour" -- every subdomain's rows by (colour, row), two sweep levels on hexahedral and MINC
        meshes; what it does not combine with (asm, ILU(k), sub lu, network blocks in the factor) is refused by the next set-up"""
        if ordering not in _lib.PC_ORDER:
            raise ValueError("pc ordering %r: one of %s" % (ordering, sorted(_lib.PC_ORDER)))
        self._chk(LIB.wai_set_pc_ordering(self.h, _lib.PC_ORDER[ordering]), "set_pc_ordering")

    def pc_ordering(self):
        """(ordering, max_colours): the setting, and the most colours of any subdomain -- 0 before a set-up under multicolour"""
        o, m = C.c_int(0), C.c_int(0)
        self._chk(LIB.wai_get_pc_ordering(self.h, C.byref(o), C.byref(m)), "pc_ordering")
        return {v: k for k, v in _lib.PC_ORDER.items()}[o.value], m.value

    def set_pc_coarse(self, mode, aggregates=None, boxes=None):
        """a coarse level for the flow system's preconditioner (wai_set_pc_coarse): mode "additive", "deflated" or "off"
        (also None / False).  aggregates: the 0-based aggregate of every owned cell; or boxes=(nx, ny, nz) on a structured
        mesh: the mesh cut into that many boxes per axis (box_aggregates).  One level, piecewise constant, Galerkin, the
        coarse matrix inverted densely on the device: at most 1024 / block size aggregates.  What it does not combine with
        is refused by name, and what was in force stays in force"""
        mode = "off" if mode in (None, False) else mode
        if mode not in _lib.PC_COARSE:
            raise ValueError("pc coarse mode %r: one of %s" % (mode, sorted(_lib.PC_COARSE)))
        if mode == "off":
            self._chk(LIB.wai_set_pc_coarse(self.h, 0, 0, None), "set_pc_coarse")
            return
        if (aggregates is None) == (boxes is None):
            raise ValueError("set_pc_coarse: give either aggregates or boxes")
        if boxes is not None:
            if getattr(self.mesh, "owned_ijk", None) is None:
                raise ValueError("set_pc_coarse: boxes need a structured mesh (owned_ijk); give aggregates")
            aggregates = box_aggregates(self.mesh.owned_ijk, boxes)
        agg = _lib._i32(aggregates)
        if agg.size != self.n_owned:
            raise ValueError("set_pc_coarse: %d aggregates for %d owned cells" % (agg.size, self.n_owned))
        nc = int(agg.max()) + 1 if agg.size else 0
        self._chk(LIB.wai_set_pc_coarse(self.h, _lib.PC_COARSE[mode], nc, agg.ctypes.data_as(_lib.pi)), "set_pc_coarse")

    def pc_coarse(self):
        """(mode, nc): the coarse level's setting and its number of aggregates, ("off", 0) by default"""
        m, nc = C.c_int(0), C.c_int(0)
        self._chk(LIB.wai_get_pc_coarse(self.h, C.byref(m), C.byref(nc)), "pc_coarse")
        return {v: k for k, v in _lib.PC_COARSE.items()}[m.value], nc.value

    def test_coarse(self, what, vin, out):
        """one piece of the coarse level alone (wai_test_coarse): what is a key of lib.COARSE_WHAT; vin / out are float64
        numpy arrays or torch tensors on the device, out written in place; returns the library's code (1: a pivot failed)"""
        return self._chk(LIB.wai_test_coarse(self.h, _lib.COARSE_WHAT[what], None if vin is None else _lib.ptr(vin), _lib.ptr(out)),
                         "test_coarse")

    def set_pc_tiles(self, tile_ptr):
        """tiles of the preconditioner's subdomains (wai_set_pc_tiles): contiguous owned-row ranges of 1 .. 1024 rows from 0 to
        n_owned that refine the subdomains -- the mesh's bricks under one block per rank.  A subdomain of more than 1024 rows then
        runs its substitution sweeps with one launch per level of tiles where that is fewer launches; None clears the tiles"""
        if tile_ptr is None:
            self._chk(LIB.wai_set_pc_tiles(self.h, 0, None), "set_pc_tiles")
            self.pc_tiles = None
            return
        tp = _lib._i32(tile_ptr)
        self._chk(LIB.wai_set_pc_tiles(self.h, tp.size - 1, tp.ctypes.data_as(_lib.pi)), "set_pc_tiles")
        self.pc_tiles = tp

    def tile_schedule(self, extended=False):
        """the tile schedule of the flow system's preconditioner as set up now (wai_test_tile_schedule): a dict of tiles, ntl_f,
        ntl_b, max_tile_rows, max_in_levels, serve, nlev_f, nlev_b; extended: of the extended system (PCASM, ILU(k))"""
        f = (C.c_int * 8)()
        self._chk(LIB.wai_test_tile_schedule(self.h, 1 if extended else 0, f), "test_tile_schedule")
        return dict(zip("tiles ntl_f ntl_b max_tile_rows max_in_levels serve nlev_f nlev_b".split(), list(f)))

    def aux_block_system(self, method, dt, ratio, alx_last, alx_last2):
        """(values (nnzb, nt): the diagonals of the coupled system's blocks on setup_jacobian()'s pattern, rhs
        (n_owned * nt) interleaved [cell][tracer])"""
        nnzb = LIB.wai_jacobian_nnzb(self.h)
        val, b = np.zeros((nnzb, self.num_tracers)), np.zeros(self.n_owned * self.num_tracers)
        self._chk(LIB.wai_tracer_block_system(self.h, _lib.METHOD_KIND[method], dt, ratio, _lib.ptr(alx_last),
                                              _lib.ptr(alx_last2), val.ctypes.data, b.ctypes.data), "tracer_block_system")
        return val, b

    def tracer_assembly_sweeps(self):
        """tracer assembly sweeps over the faces so far (nt per per-tracer solve, one per coupled solve)"""
        a = C.c_longlong(0)
        self._chk(LIB.wai_tracer_stats(self.h, C.byref(a)), "tracer_stats")
        return a.value

    def set_aux_solver(self, ksp_type="gmres", restart=30, rtol=1e-5, atol=1e-50, max_its=10000):
        """the auxiliary (tracer) KSP: "gmres" (default), "bcgs", "lgmres" or "bcgsl" (the last two per tracer only: the
        coupled solve refuses them)"""
        return self._chk(LIB.wai_set_aux_solver(self.h, _lib.KSP[ksp_type], restart, rtol, atol,
                                                max_its), "set_aux_solver")

    def set_aux_pc(self, pc_type="follow", asm_overlap=1, ilu_levels=0, sub_pc="ilu"):
        """the tracer solves' own preconditioner (wai_set_aux_pc): "bjacobi" (the reference's auxiliary default), "asm",
        "none", "lu", or "follow" (default): the flow solver's pc_type, ilu_levels and sub-preconditioner"""
        self._chk(LIB.wai_set_aux_pc(self.h, _lib.AUX_PC[pc_type] if isinstance(pc_type, str) else int(pc_type), int(asm_overlap),
                                     int(ilu_levels), _lib.SUB_PC[sub_pc] if isinstance(sub_pc, str) else int(sub_pc)), "set_aux_pc")

    def get_aux_pc(self):
        """dict(pc_type, asm_overlap, ilu_levels, sub_pc) as set_aux_pc takes them; pc_type "follow" on a fresh context"""
        v = [C.c_int(0) for _ in range(4)]
        self._chk(LIB.wai_get_aux_pc(self.h, *[C.byref(x) for x in v]), "get_aux_pc")
        name = {n: k for k, n in _lib.AUX_PC.items()}
        sub = {n: k for k, n in _lib.SUB_PC.items()}
        return dict(pc_type=name[v[0].value], asm_overlap=v[1].value, ilu_levels=v[2].value, sub_pc=sub[v[3].value])

    def aux_lhs(self, t, interval, Al):
        return self._chk(LIB.wai_tracer_lhs(self.h, _lib.ptr(Al)), "tracer_lhs")

    def aux_system(self, tracer, method, dt, ratio, alx_last, alx_last2):
        """(scalar CSR values on setup_jacobian()'s pattern, rhs) of one tracer's system"""
        nnzb = LIB.wai_jacobian_nnzb(self.h)
        val, b = np.zeros(nnzb), np.zeros(self.n_owned)
        self._chk(LIB.wai_tracer_system(self.h, tracer, _lib.METHOD_KIND[method], dt, ratio, _lib.ptr(alx_last),
                                        _lib.ptr(alx_last2), val.ctypes.data, b.ctypes.data), "tracer_system")
        return val, b

    def aux_solve(self, method, dt, ratio, alx_last, alx_last2, X, alx_new):
        """setup_linear + aux_pre_solve + KSPSolve (timestepper.F90:2345-2355); (reason, its)"""
        its, reason = C.c_int(0), C.c_int(0)
        self._chk(LIB.wai_tracer_solve(self.h, _lib.METHOD_KIND[method], dt, ratio, _lib.ptr(alx_last),
                                       _lib.ptr(alx_last2), _lib.ptr(X), _lib.ptr(alx_new), C.byref(its),
                                       C.byref(reason)), "tracer_solve")
        return reason.value, its.value

    # ---- measurement ---------------------------------------------------------------------------
    def timer_start(self):
        self._chk(LIB.wai_timer_start(self.h), "timer_start")

    def timer_stop(self):
        ms = C.c_float(0)
        self._chk(LIB.wai_timer_stop(self.h, C.byref(ms)), "timer_stop")
        return ms.value

    def bench_kernel(self, which, reps=100):
        ms = C.c_float(0)
        self._chk(LIB.wai_bench_kernel(self.h, which, reps, C.byref(ms)), "bench_kernel")
        return ms.value

    def synchronize(self):
        self._chk(LIB.wai_synchronize(self.h), "synchronize")

    def profile(self, on=True):
        LIB.wai_profile_enable(self.h, 1 if on else 0)
        LIB.wai_profile_reset(self.h)

    def profile_get(self):
        out = {}
        for k, name in enumerate(_lib.KCLASS):
            ms, n = C.c_double(0), C.c_longlong(0)
            LIB.wai_profile_get(self.h, k, C.byref(ms), C.byref(n))
            out[name] = (ms.value, n.value)
        return out
