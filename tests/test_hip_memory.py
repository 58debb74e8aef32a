"""Who frees device memory: every buffer of a context has one owner (DevBuf, csrc/devbuf.hpp) and no free list is kept,
so what the library's counter of live device allocations (wai_test_device_memory) reads is the check -- a destroyed
context returns everything it allocated on any path, setting things again does not grow it, and a context whose
creation was refused half-way can be destroyed.  Every assertion compares the counter with its own reading at the
start of the test: other fixtures may hold contexts."""
import ctypes as C

import numpy as np
import pytest

from tests.test_hip_pc import system
from waiwera_amd import lib as wl
from waiwera_amd.cases import make_case, scaled

pytestmark = pytest.mark.gpu
DIMS, BRICK, DT = (6, 6, 4), (3, 3, 2), 5.0e4
DECAY, ACT, DIFF = [1e-8, 1e-7, 2e-7], [0.0, 0.0, 1.5e3], [1e-6, 2e-5, 0.0]


def network(lm):
    """the producers on deliverability in one limited group behind a separator, whose water feeds two injectors: their
    rates depend on each other's cells, which is what gives the network Jacobian blocks (after
    tests/test_hip_multirank.py::_network_spec)"""
    rate = np.asarray(lm.src_rate)
    prod = [int(i) for i in np.flatnonzero(rate < 0)]
    inj = [int(i) for i in np.flatnonzero((rate > 0) & (np.asarray(lm.src_component) == 1))]      # the water injectors
    controls = [dict(kind="deliverability", coef=1.0e-11, pressure=2.0e5) if r < 0 else dict() for r in rate]
    spec = dict(rate_specified=[1] * len(rate), enthalpy_specified=[int(r > 0) for r in rate],
                groups=[dict(inputs=[(1, i) for i in prod], scaling=0, limits=[(0, 12.0)], separator=[(640.0e3, 2748.0e3)])],
                reinjectors=[dict(input=(2, 0), overflow=(0, -1),
                                  outputs=[dict(flow=1, out=(1, inj[0]), rate=-1.0, proportion=0.5, enthalpy=-1.0),
                                           dict(flow=1, out=(1, inj[-1]), rate=-1.0, proportion=0.3, enthalpy=-1.0)])])
    return controls, spec


def set_sources(sim, lm):
    sc, sr = wl._i32(lm.src_cell), wl._f64(lm.src_rate)
    se, sk = wl._f64(lm.src_enthalpy), wl._i32(lm.src_component)
    sim._chk(wl.LIB.wai_set_sources(sim.h, sc.size, sc.ctypes.data_as(wl.pi), sr.ctypes.data_as(wl.pd),
                                    se.ctypes.data_as(wl.pd), sk.ctypes.data_as(wl.pi)), "set_sources")


class Tracers:
    """nt tracers on sim, with boundary values and injection, and the vectors a solve needs"""

    def __init__(self, sim, lm, nt):
        rng = np.random.default_rng(5)
        self.sim, self.n = sim, lm.n_owned * nt
        self.inj = np.where(np.asarray(lm.src_rate)[:, None] > 0, rng.uniform(0, 1e-2, (lm.n_src, nt)), 0.0)
        sim.set_tracers([0, 1, 0][:nt], DECAY[:nt], ACT[:nt], DIFF[:nt], bc=rng.uniform(0, 1e-3, (lm.n_bc, nt)), injection=self.inj)
        self.X0 = rng.uniform(0, 1e-3, self.n)
        Al = np.zeros(self.n)
        sim.aux_lhs(0.0, None, Al)
        self.alx = Al * self.X0

    def solve(self, mode):
        self.sim.set_tracer_solve_mode(mode)
        X, new = self.X0.copy(), np.zeros(self.n)
        reason, its = self.sim.aux_solve("beuler", 1.0e3, 1.0, self.alx, self.alx, X, new)
        assert reason > 0 and np.isfinite(X).all()


def flow_solve(sim, f, **opts):
    sim.set_opts(**opts)
    x = np.zeros(sim.num_dof)
    its, reason, rn = sim.ksp_solve(f, x)
    assert reason > 0 and np.isfinite(x).all()


def state(eos):
    g, lm, prim, region = make_case(dims=DIMS, brick=BRICK, eos=eos, lens=(eos == "we"))
    return scaled(prim, region, eos).ravel().copy()


@pytest.mark.parametrize("eos", ["we", "wce"])
def test_destroy_returns_everything(oracle, eos):
    """every allocation path driven on one context (and the level-set schedule of one-block subdomains on a second):
    after destroy() the counter reads what it read before"""
    start = wl.device_memory()
    lm, sim, osim, J, f = system(oracle, eos, DIMS, BRICK, lens=(eos == "we"))
    assert wl.device_memory()[0] > start[0] and wl.device_memory()[1] > start[1]
    n = sim.num_dof
    flow_solve(sim, f, ksp_type="bcgs")
    flow_solve(sim, f, ksp_type="gmres")                     # the basis
    flow_solve(sim, f, ksp_type="lgmres")
    flow_solve(sim, f, ksp_type="bcgsl")
    for overlap in (1, 2):                                   # the extended system, rebuilt
        sim.set_opts(pc_type="asm", asm_overlap=overlap)
        assert sim.pc_setup() == 0
    sim.set_opts(pc_type="bjacobi", asm_overlap=1, ilu_levels=1)
    assert sim.pc_setup() == 0
    sim.set_opts(ilu_levels=0)
    sim.set_sub_pc("lu")
    for pc in ("bjacobi", "asm"):
        sim.set_opts(pc_type=pc)
        assert sim.pc_setup() == 0
    sim.set_sub_pc("ilu")
    sim.set_opts(pc_type="lu")
    assert sim.pc_setup() == 0
    sim.set_opts(pc_type="bjacobi", ksp_type="bcgs")
    # sources are the mesh's; controls and a network on them, its Jacobian blocks, and those inside the factor's pattern
    y = state(eos)
    controls, spec = network(lm)
    sim.set_source_controls(controls)
    sim.set_source_network(spec)
    L, r = np.zeros(n), np.zeros(n)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, (0.0, 0.0), y, L)
    assert sim.residual(0.0, DT, y, L, r) == 0
    assert sim.jacobian(0.0, DT, y, L) == 0
    cells, E = sim.network_couplings()
    assert len(cells) > 0 and np.abs(E).max() > 0
    for pc in ("bjacobi", "asm"):
        sim.set_opts(pc_type=pc)
        assert sim.pc_setup() >= 0
    sim.set_opts(pc_type="bjacobi")
    assert len(sim.fluxes()) and len(sim.source_rates()[0]) == lm.n_src
    assert sim.separator_enthalpies(5.0e5)[1] > 0
    sim.set_jacobian_values(sim.jacobian_values())
    tr = Tracers(sim, lm, 2)
    tr.solve("per_tracer")
    tr.solve("coupled")
    sim.destroy(); osim.close()
    # subdomains of any size: the level sets of the launch-per-level path
    lm, sim, osim, J, f = system(oracle, eos, DIMS, DIMS, one_block=True, lens=(eos == "we"))
    flow_solve(sim, f, ksp_type="bcgs")
    sim.destroy(); osim.close()
    assert wl.device_memory() == start


def test_reconfiguring_does_not_grow(oracle):
    """one cycle of setting everything again settles every buffer's size; three more leave allocations and bytes as they are"""
    lm, sim, osim, J, f = system(oracle, "we", DIMS, BRICK)
    controls, _ = network(lm)

    def cycle():
        for nt in (2, 3, 2):
            tr = Tracers(sim, lm, nt)
            sim.set_tracer_injection(tr.inj)
            tr.solve("coupled")
            tr.solve("per_tracer")
        set_sources(sim, lm)
        sim.set_source_controls(controls)
        for pc in ("asm", "bjacobi"):
            sim.set_opts(pc_type=pc)
            assert sim.pc_setup() == 0
        for sub in ("lu", "ilu"):
            sim.set_sub_pc(sub)
            assert sim.pc_setup() == 0
        for restart in (10, 30):
            flow_solve(sim, f, ksp_type="gmres", gmres_restart=restart)

    assert sim.pre_eval(0.0, state("we")) == 0      # the fluid state the tracer systems are assembled on
    cycle()
    settled = wl.device_memory()
    for _ in range(3):
        cycle()
    assert wl.device_memory() == settled
    sim.destroy(); osim.close()


def mesh_desc(lm, face_cells, face_geom):
    keep = (wl._i32(face_cells), wl._f64(face_geom), wl._f64(lm.cell_geom), wl._f64(lm.rock), wl._i32(lm.sub_ptr))
    md = wl.MeshDesc()
    md.n_owned, md.n_halo, md.n_bc, md.n_faces = lm.n_owned, lm.n_halo, lm.n_bc, len(keep[0]) // 2
    md.face_cells, md.face_geom = keep[0].ctypes.data_as(wl.pi), keep[1].ctypes.data_as(wl.pd)
    md.cell_geom, md.rock = keep[2].ctypes.data_as(wl.pd), keep[3].ctypes.data_as(wl.pd)
    md.n_sub, md.sub_ptr = keep[4].size - 1, keep[4].ctypes.data_as(wl.pi)
    return md, keep


@pytest.mark.parametrize("why", ["duplicate connection", "unsupported eos kind"])
def test_a_refused_creation_is_destroyable(why):
    """a mesh with the same connection twice is refused after the geometry is on the device, an unknown EOS before
    anything is: wai_ctx_destroy on the handle either returns gives everything back"""
    start = wl.device_memory()
    g, lm, prim, region = make_case(dims=DIMS, brick=BRICK, eos="we")
    fc, fg = np.asarray(lm.face_cells).reshape(-1, 2), np.asarray(lm.face_geom).reshape(-1, 12)
    eos = wl.eos_desc("we")
    if why == "duplicate connection":
        twice = int(np.flatnonzero((fc < lm.n_owned).all(axis=1))[0])      # a face between two owned cells, once more
        fc, fg = np.vstack([fc, fc[twice:twice + 1]]), np.vstack([fg, fg[twice:twice + 1]])
    else:
        eos.kind = 99
    md, keep = mesh_desc(lm, fc.ravel(), fg.ravel())
    opts, h = wl.default_opts(), C.c_void_p()
    assert wl.LIB.wai_ctx_create(C.byref(md), C.byref(eos), C.byref(opts), 0, C.byref(h)) == -2
    assert h and why in wl.LIB.wai_last_error(h).decode()
    held = wl.device_memory()
    assert (held[0] > start[0]) == (why == "duplicate connection")
    assert wl.LIB.wai_ctx_destroy(h) == 0
    assert wl.device_memory() == start
