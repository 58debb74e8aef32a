"""The coupled tracer solve (wai_set_tracer_solve_mode, WAI_TRACER_COUPLED): all nt tracers in ONE left-preconditioned
Krylov solve on the [cell][tracer] vector, as the reference's auxiliary KSPSolve (src/timestepper.F90:2345-2355) -- the
system against the per-tracer systems, the solve against the oracle's block Krylov solver on the same system (block size
nt, diagonal blocks) and against direct solves, its semantics, its launch structure, what it refuses, whole runs.

Tolerances: 1e-8 of the largest entry against the oracle's solve of the same system (tests/test_hip_pc.py's solution
tolerance), iteration counts within one ("within rounding", the same file); 1e-7 against a direct solve at rtol 1e-12 (what
tests/test_hip_tracer.py::test_tracer_solve_parity applies to the per-tracer path)."""
import os

import numpy as np
import pytest

from oracle import binding as ol
from tests.tracer_block_reference import block_values, csr_of, direct_solutions
from waiwera_amd.cases import make_case, scaled

pytestmark = pytest.mark.gpu
KIND = {"w": 0, "we": 1, "wce": 2}
PHASES = [0, 1, 0, 1, 1, 0, 0, 1]
DECAY = [1e-8, 1e-7, 2e-7, 3e-8, 5e-8, 4e-7, 6e-8, 9e-8]
ACT = [0.0, 0.0, 1.5e3, 0.0, 2.0e3, 0.0, 5.0e2, 0.0]
DIFF = [1e-6, 2e-5, 0.0, 3e-6, 1e-5, 0.0, 2e-6, 4e-6]
METHODS = ("beuler", "bdf2", "directss")


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class Case:
    """a converged flow step on a small mesh with nt tracers of different phases, decay constants, activation energies
    and diffusion coefficients; the we lens and the wce column leave cells without the vapour phase"""

    def __init__(self, eos="we", nt=2, one_block=False, wide=False, zero_first=False, seed=11):
        from waiwera_amd.flow_simulation import FlowSimulation
        if wide:
            from tests.wide_mesh import wide_case
            lm, prim, region, _ = wide_case(eos)
        else:
            g, lm, prim, region = make_case(eos=eos, dims=(8, 7, 9), brick=(4, 7, 3), lens=(eos == "we"))
        self.sub_ptr = None if lm.sub_ptr is None else np.array(lm.sub_ptr)
        if one_block:
            lm.sub_ptr = None
        self.lm, self.eos, self.nt = lm, eos, nt
        self.sim = sim = FlowSimulation(lm, eos=eos)
        if one_block:
            lm.sub_ptr = np.array([0, lm.n_owned], dtype=np.int32)
        sim.set_regions(region)
        rng = np.random.default_rng(seed)
        self.phases = PHASES[:nt]
        bc = rng.uniform(0, 1e-3, (lm.n_bc, nt))
        nsrc = getattr(lm, "n_src", 0)
        inj = np.where(np.asarray(lm.src_rate)[:, None] > 0, rng.uniform(0, 1e-2, (nsrc, nt)), 0.0) if nsrc else None
        self.n = n = lm.n_owned * nt
        X0 = rng.uniform(0, 1e-3, n)
        if zero_first:   # tracer 0: nothing resident, nothing injected, nothing at the boundary -> zero right-hand side
            bc[:, 0] = 0.0
            if inj is not None:
                inj[:, 0] = 0.0
            X0[0::nt] = 0.0
        self.bc, self.inj, self.X0 = bc, inj, X0
        self.set_tracers(DECAY[:nt])
        sim.set_opts(ksp_rtol=1e-10, ftol_rel=1e-9)
        y = scaled(prim, region, eos).ravel().copy()
        assert sim.pre_eval(0.0, y) == 0
        Al = np.zeros(n)
        sim.aux_lhs(0.0, None, Al)
        self.alx1 = Al * X0
        self.alx2 = self.alx1 * (1.0 + 0.01 * rng.standard_normal(n))
        self.dt = 5.0e2 if eos == "wce" else 1.0e4
        for _ in range(5):
            reason, nits, kits = sim.timestep(0.0, self.dt, y)
            if reason > 0:
                break
            self.dt *= 0.2
        assert reason > 0
        self.y = y
        self.rowptr, self.colidx = sim.setup_jacobian()

    def set_tracers(self, decay):
        nt = self.nt
        self.sim.set_tracers(self.phases, decay, ACT[:nt], DIFF[:nt], bc=self.bc, injection=self.inj)

    def solve(self, mode, method="beuler", ksp="gmres", **kw):
        sim = self.sim
        sim.set_tracer_solve_mode(mode)
        sim.set_aux_solver(ksp, **kw)
        X, new = self.X0.copy(), np.zeros(self.n)
        reason, its = sim.aux_solve(method, self.dt, 1.3, self.alx1, self.alx2, X, new)
        return X, new, reason, its

    def block_system(self, method="beuler"):
        return self.sim.aux_block_system(method, self.dt, 1.3, self.alx1, self.alx2)


@pytest.mark.parametrize("eos,nt,wide", [("we", 2, False), ("wce", 3, False), ("we", 8, False), ("we", 5, True)])
def test_block_system_is_the_per_tracer_systems(eos, nt, wide):
    """wai_tracer_block_system equals nt calls of wai_tracer_system entry by entry, for every time stepping method:
    the one-sweep assembly does the per-tracer arithmetic (rows of up to 15 blocks on the wide mesh)"""
    c = Case(eos, nt, wide=wide)
    for method in METHODS:
        V, b = c.block_system(method)
        assert V.shape == (len(c.colidx), nt) and b.shape == (c.n,)
        for it in range(nt):
            A1, b1 = c.sim.aux_system(it, method, c.dt, 1.3, c.alx1, c.alx2)
            assert np.array_equal(V[:, it], A1), (method, it, np.abs(V[:, it] - A1).max())
            assert np.array_equal(b[it::nt], b1), (method, it)
    if 1 in c.phases and not wide:   # aux_pre_solve's identity rows, per tracer
        iv = c.phases.index(1)
        diag = np.array([np.flatnonzero(c.colidx[c.rowptr[i]:c.rowptr[i + 1]] == i)[0] + c.rowptr[i] for i in range(c.lm.n_owned)])
        ident = (V[diag, iv] == 1.0) & (b[iv::nt] == 0.0)
        assert ident.any() and not ((V[diag, 0] == 1.0) & (b[0::nt] == 0.0)).all()
    c.sim.destroy()


@pytest.mark.parametrize("eos,nt", [("we", 2), ("wce", 3)])
def test_coupled_solve_against_the_oracle_block_krylov(oracle, eos, nt):
    """nt = np: the oracle's block GMRES(30) + block-Jacobi ILU(0) (the reference arithmetic, unchanged) on the BCSR system
    of diagonal np x np blocks, rtol 1e-5, same subdomains: same reason, iteration count within one, same solution"""
    c = Case(eos, nt)
    osim = ol.OracleSim(oracle, c.lm, KIND[eos])
    V, b = c.block_system("beuler")
    oreason, xo, oits, hist = osim.ksp_solve(block_values(V).ravel(), b, ksp_type=1, restart=30, rtol=1e-5)
    X, new, reason, its = c.solve("coupled", rtol=1e-5)
    print(eos, "coupled its", its, "oracle its", oits, "reason", reason, oreason, "difference", np.abs(X - xo).max(), "of", np.abs(xo).max())
    assert reason == oreason and reason > 0
    assert abs(its - oits) <= 1
    assert np.abs(X - xo).max() <= 1e-8 * np.abs(xo).max()
    c.sim.destroy(); osim.close()


@pytest.mark.parametrize("eos,nt,ksp,pc,one_block,wide", [
    ("we", 2, "gmres", "bjacobi", False, False), ("wce", 3, "gmres", "bjacobi", False, False),
    ("we", 4, "gmres", "bjacobi", False, False), ("we", 8, "gmres", "bjacobi", False, False),
    ("we", 2, "bcgs", "bjacobi", False, False), ("we", 8, "bcgs", "bjacobi", False, False),
    ("wce", 3, "gmres", "bjacobi", True, False), ("we", 5, "bcgs", "bjacobi", True, False),
    ("we", 3, "gmres", "bjacobi", False, True), ("we", 8, "bcgs", "bjacobi", False, True),
    ("we", 2, "gmres", "none", False, False)])
def test_coupled_solve_against_direct_solves(eos, nt, ksp, pc, one_block, wide):
    """rtol 1e-12: the coupled solution against scipy's direct solve of each tracer's system -- bricks, one block per rank
    (the launch-per-level path), rows of 9 .. 16 blocks, GMRES and BiCGStab, nt = 4 and 8 (the chunked kernels)"""
    c = Case(eos, nt, one_block=one_block, wide=wide)
    c.sim.set_opts(pc_type=pc)
    for method in METHODS:
        if method == "directss":   # a decay rate above the flushing rate: a well-conditioned steady state (test_hip_tracer.py)
            c.set_tracers([1e-3 * (1 + t) for t in range(nt)])
        V, b = c.block_system(method)
        X, new, reason, its = c.solve("coupled", method, ksp, rtol=1e-12)
        xs = direct_solutions(c.rowptr, c.colidx, V, b)
        print(eos, nt, ksp, pc, method, "its", its, "reason", reason, "against direct", relmax(X, xs))
        assert reason > 0, (method, reason)
        if pc == "none":
            # no preconditioner: the test is on the residual itself, 1e-12 |b|; two digits for the recursive residual's drift
            res = np.concatenate([(csr_of(c.rowptr, c.colidx, V[:, t]) @ X[t::nt] - b[t::nt]) for t in range(nt)])
            assert np.linalg.norm(res) <= 1e-10 * np.linalg.norm(b)
        else:
            assert relmax(X, xs) < 1e-7, method
        Al = np.zeros(c.n)
        c.sim.aux_lhs(0.0, None, Al)
        assert np.array_equal(new, Al * X)
    c.sim.destroy()


def test_combined_norm_one_count_and_mode_switches(oracle):
    """a tracer with a zero right-hand side beside one with a large one: ONE solve, converged on the combined norm -- the
    oracle's block solve's count; one tracer alone is bit-identical in both modes; switching back restores the per-tracer
    results bitwise"""
    c = Case("we", 2, zero_first=True)
    V, b = c.block_system("beuler")
    assert not b[0::2].any() and b[1::2].any()
    osim = ol.OracleSim(oracle, c.lm, KIND["we"])
    oreason, xo, oits, hist = osim.ksp_solve(block_values(V).ravel(), b, ksp_type=1, restart=30, rtol=1e-5)
    Xp, newp, rp, ip = c.solve("per_tracer", rtol=1e-5)
    Xc, newc, rc, ic = c.solve("coupled", rtol=1e-5)
    assert rc == oreason and abs(ic - oits) <= 1
    assert np.abs(Xc - xo).max() <= 1e-8 * np.abs(xo).max()
    assert not Xc[0::2].any()
    Xq, newq, rq, iq = c.solve("per_tracer", rtol=1e-5)
    assert np.array_equal(Xq, Xp) and np.array_equal(newq, newp) and (rq, iq) == (rp, ip)
    print("zero beside large: coupled its", ic, "oracle block its", oits, "per-tracer sum", ip)
    c.sim.destroy(); osim.close()
    # two tracers that both have something to solve: the per-tracer count is a SUM of two solves' counts (each at least
    # one), the coupled count is one solve's -- the oracle block solve's, and below the sum
    c = Case("we", 2)
    osim = ol.OracleSim(oracle, c.lm, KIND["we"])
    V, b = c.block_system("beuler")
    assert b[0::2].any() and b[1::2].any()
    oreason, xo, oits, hist = osim.ksp_solve(block_values(V).ravel(), b, ksp_type=1, restart=30, rtol=1e-5)
    ip = c.solve("per_tracer", rtol=1e-5)[3]
    ic = c.solve("coupled", rtol=1e-5)[3]
    print("both non-zero: coupled its", ic, "oracle block its", oits, "per-tracer sum", ip)
    assert abs(ic - oits) <= 1 and ic < ip
    c.sim.destroy(); osim.close()
    one = Case("we", 1)
    a = one.solve("per_tracer", rtol=1e-8)
    bq = one.solve("coupled", rtol=1e-8)
    assert np.array_equal(a[0], bq[0]) and np.array_equal(a[1], bq[1]) and a[2:] == bq[2:]
    one.sim.destroy()


@pytest.mark.parametrize("ksp,one_block", [("gmres", False), ("bcgs", False), ("gmres", True)])
def test_launches_and_reads_do_not_depend_on_nt(ksp, one_block):
    """with the iteration count forced by max_its, a coupled solve at nt = 2 and at nt = 8 launches the same kernels and
    makes the same scalar reads; one assembly sweep per coupled solve, nt per per-tracer solve"""
    counts = {}
    for nt in (2, 8):
        c = Case("we", nt, one_block=one_block)
        sim = c.sim
        c.solve("coupled", "beuler", ksp, rtol=1e-30, max_its=4)   # buffers allocated, kernels loaded
        k0, c0 = sim.launch_stats()
        s0 = sim.tracer_assembly_sweeps()
        X, new, reason, its = c.solve("coupled", "beuler", ksp, rtol=1e-30, max_its=4)
        k1, c1 = sim.launch_stats()
        assert sim.tracer_assembly_sweeps() - s0 == 1
        assert (reason, its) == (-3, 4)
        counts[nt] = (k1 - k0, c1 - c0)
        s0 = sim.tracer_assembly_sweeps()
        c.solve("per_tracer", "beuler", ksp, rtol=1e-30, max_its=4)
        assert sim.tracer_assembly_sweeps() - s0 == nt
        sim.destroy()
    print(ksp, "one block" if one_block else "bricks", "(launches, copies) of a coupled solve:", counts)
    assert counts[2] == counts[8] and counts[2][0] > 0


def test_uncovered_combinations_are_refused():
    """asm, lu and ILU(1) under the coupled mode: the solve returns -2 and a text that names the combination, never a
    per-tracer run; the system alone (no solve) is still to be had; the context is usable afterwards"""
    from waiwera_amd.flow_simulation import WaiError
    c = Case("we", 2)
    sim = c.sim
    sim.set_tracer_solve_mode("coupled")
    sim.set_aux_solver("gmres", rtol=1e-12)
    V, b = c.block_system("beuler")
    for kw, word in ((dict(pc_type="asm"), "asm"), (dict(pc_type="lu"), "lu"), (dict(pc_type="bjacobi", ilu_levels=1), "ILU(k)")):
        sim.set_opts(**kw)
        s0 = sim.tracer_assembly_sweeps()
        with pytest.raises(WaiError) as e:
            sim.aux_solve("beuler", c.dt, 1.0, c.alx1, None, c.X0.copy(), np.zeros(c.n))
        assert "(-2)" in str(e.value) and word in str(e.value) and "coupled" in str(e.value), str(e.value)
        assert sim.tracer_assembly_sweeps() == s0
        V2, b2 = c.block_system("beuler")
        assert np.array_equal(V2, V) and np.array_equal(b2, b)
        sim.set_opts(pc_type="bjacobi", ilu_levels=0)
    X, new, reason, its = c.solve("coupled", rtol=1e-12)
    assert reason > 0 and relmax(X, direct_solutions(c.rowptr, c.colidx, V, b)) < 1e-7
    assert sim.timestep(c.dt, c.dt, c.y)[0] > 0   # the flow solver on its own matrix, vectors and factor again
    sim.destroy()


@pytest.mark.parametrize("eos,nt,wide", [("wce", 3, False), ("we", 4, True), ("we", 8, False)])
def test_timestepper_run_coupled_equals_per_tracer(eos, nt, wide):
    """three BDF2 steps through the Timestepper (the small box; the mesh of 9 .. 16-face cells; eight tracers): the coupled
    run's tracer fields equal the per-tracer run's to the solves' tolerance (rtol 1e-12 each: 1e-7 as against a direct solve)"""
    from waiwera_amd.timestepper import Timestepper
    out = {}
    for mode in ("per_tracer", "coupled"):
        c = Case(eos, nt, wide=wide)
        c.sim.set_aux_solver("gmres", rtol=1e-12)
        X = c.X0.copy()
        assert c.sim.pre_eval(0.0, c.y) == 0
        ts = Timestepper(c.sim, c.y, stepsize=c.dt, method="bdf2", aux_solution=X, tracer_solve_mode=mode)
        ts.init_auxiliary()
        ts.run(3)
        assert ts.taken == 3 and all(r > 0 for r, _ in ts.aux_history)
        out[mode] = (X.copy(), list(ts.aux_history))
        c.sim.destroy()
    print("aux (reason, its) per step: per tracer", out["per_tracer"][1], "coupled", out["coupled"][1])
    assert relmax(out["coupled"][0], out["per_tracer"][0]) < 1e-7


def test_reference_tracer_benchmarks_through_the_front_end(tmp_path):
    """tracer/oned (two-phase) and tracer/doublet with Simulation(..., tracer_solve="coupled"), against the same golden data
    with the tolerances of tests/test_hip_input.py (one tracer each: the mode's single-tracer path)"""
    import shutil
    from tests import benchmarks as B
    from waiwera_amd.simulation import Simulation
    inputs = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
    for f in ("oned_two_phase.json", "oned_two_phase_ss.h5", "goned.msh"):
        shutil.copy(os.path.join(inputs, f), tmp_path / f)
    sim = Simulation.from_json(str(tmp_path / "oned_two_phase.json"), tracer_solve="coupled")
    assert sim.ode.tracer_solve_mode == "coupled"
    out = sim.run()
    a = B.load_tracer_oned()["cases"]["two"]["autough2_final_table"]
    eX = np.abs(out["tracer_tracer"] - np.asarray(a["Tracer/liquid"]))
    assert np.all((eX <= 1.0e-3 * np.asarray(a["Tracer/liquid"])) | (eX <= 1.0e-4))
    assert (np.abs(out["fluid_pressure"] - a["Pressure"]) / np.asarray(a["Pressure"])).max() < 1.0e-3
    sim.ode.destroy()
    sim = Simulation.from_json(os.path.join(inputs, "doublet.json"), tracer_solve="coupled")
    out = sim.run()
    fx = B.load_fixture("benchmark_tracer_doublet.json")
    worst_field, worst_flow, matched = B.doublet_errors(sim, fx)
    assert matched >= 17 and worst_field < 1.0e-3 and worst_flow < 1.0e-3
    Pa = np.asarray(fx["pressure"])
    assert (np.abs(out["fluid_pressure"] - Pa) / Pa).max() < 1.0e-4
    sim.ode.destroy()
    with pytest.raises(ValueError):
        Simulation.from_json(os.path.join(inputs, "doublet.json"), tracer_solve="both")


def test_two_tracers_through_the_front_end(tmp_path):
    """tracer/oned (two-phase) with its tracer entered twice: a coupled whole run through the input front end, both
    tracers against the benchmark's AUTOUGH2 table at its 1e-3; under the front end's default preconditioner (asm, the
    reference's) the combination is refused when the simulation is set up, by keyword"""
    import json
    import shutil
    from tests import benchmarks as B
    from waiwera_amd.simulation import Simulation
    inputs = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
    for f in ("oned_two_phase.json", "oned_two_phase_ss.h5", "goned.msh"):
        shutil.copy(os.path.join(inputs, f), tmp_path / f)
    inp = json.load(open(tmp_path / "oned_two_phase.json"))
    inp["tracer"] = [{"name": "first"}, {"name": "second"}]
    with pytest.raises(ValueError, match="default_pc='bjacobi'"):
        Simulation(inp, base_dir=str(tmp_path), tracer_solve="coupled")
    sim = Simulation(inp, base_dir=str(tmp_path), tracer_solve="coupled", default_pc="bjacobi")
    s0 = sim.ode.tracer_assembly_sweeps()
    out = sim.run()
    assert sim.ode.tracer_assembly_sweeps() - s0 == len(sim.ts.aux_history) > 0    # one sweep per step: the coupled path ran
    a = B.load_tracer_oned()["cases"]["two"]["autough2_final_table"]
    Xa = np.asarray(a["Tracer/liquid"])
    for name in ("first", "second"):
        eX = np.abs(out["tracer_" + name] - Xa)
        assert np.all((eX <= 1.0e-3 * Xa) | (eX <= 1.0e-4)), name
    assert (np.abs(out["fluid_pressure"] - a["Pressure"]) / np.asarray(a["Pressure"])).max() < 1.0e-3
    sim.ode.destroy()
