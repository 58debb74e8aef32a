"""The auxiliary (tracer) solver's own preconditioner (wai_set_aux_pc) and its further Krylov types: "follow" is the default
and is the behaviour before the setting existed; a setting of its own acts on the tracer solves alone, in any order of flow
and tracer solves; the coupled solve tests the AUXILIARY preconditioner, so the reference's defaults -- flow asm, tracers
under block Jacobi -- are covered; lgmres and bcgsl per tracer.

The problem is tests/test_hip_tracer_coupled.py's: 8 x 7 x 9 cells in six bricks of 4 x 7 x 3, so that an overlapped block
of asm reaches into its neighbours.  Tolerances are that file's: 1e-7 against a direct solve at rtol 1e-12; against the
oracle's block GMRES at rtol 1e-5 the same reason, the iteration count within one, 1e-8 of the largest entry."""
import numpy as np
import pytest

from oracle import binding as ol
from tests.test_hip_tracer_coupled import KIND, Case, relmax
from tests.tracer_block_reference import block_values, direct_solutions

pytestmark = pytest.mark.gpu


def reset(sim):
    sim.set_opts(pc_type="bjacobi", asm_overlap=1, ilu_levels=0)
    sim.set_sub_pc("ilu")
    sim.set_aux_pc("follow")
    sim.set_tracer_solve_mode("per_tracer")


@pytest.fixture(scope="module")
def case():
    """we, nt = 2: one converged flow step, shared; every test leaves the settings as it found them (reset)"""
    c = Case("we", 2)
    c.V, c.b = c.block_system("beuler")
    c.xs = direct_solutions(c.rowptr, c.colidx, c.V, c.b)
    yield c
    c.sim.destroy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_follow_is_the_default_and_is_the_flow_solvers_preconditioner(case):
    """a fresh context reports follow; naming the flow solver's own settings explicitly changes nothing, bit for bit, per
    tracer and coupled, under bjacobi and under asm (where the coupled mode is refused alike)"""
    from waiwera_amd.flow_simulation import WaiError
    c, sim = case, case.sim
    assert sim.get_aux_pc() == dict(pc_type="follow", asm_overlap=1, ilu_levels=0, sub_pc="ilu")
    for pc in ("bjacobi", "asm"):
        sim.set_opts(pc_type=pc, asm_overlap=1)
        modes = ("per_tracer", "coupled") if pc == "bjacobi" else ("per_tracer",)
        follow = {m: c.solve(m, rtol=1e-12) for m in modes}
        sim.set_aux_pc(pc, 1, 0, "ilu")
        assert sim.get_aux_pc()["pc_type"] == pc
        for m in modes:
            named = c.solve(m, rtol=1e-12)
            assert follow[m][2] > 0 and same(named, follow[m]), (pc, m, follow[m][2:], named[2:])
        if pc == "asm":
            texts = []
            for setting in (("follow",), ("asm", 1, 0, "ilu")):
                sim.set_aux_pc(*setting)
                sim.set_tracer_solve_mode("coupled")
                with pytest.raises(WaiError) as e:
                    sim.aux_solve("beuler", c.dt, 1.3, c.alx1, c.alx2, c.X0.copy(), np.zeros(c.n))
                texts.append(str(e.value))
            assert texts[0] == texts[1] and "(-2)" in texts[0] and "asm" in texts[0]
        sim.set_aux_pc("follow")
    assert sim.get_aux_pc()["pc_type"] == "follow"
    with pytest.raises(WaiError) as e:
        sim.set_aux_pc(9)
    assert "(-2)" in str(e.value) and "auxiliary preconditioner" in str(e.value)
    for bad in (dict(ilu_levels=9), dict(sub_pc=5)):
        with pytest.raises(WaiError) as e:
            sim.set_aux_pc("bjacobi", **bad)
        assert "(-2)" in str(e.value)
    assert sim.get_aux_pc()["pc_type"] == "follow"
    reset(sim)


def test_the_setting_acts_and_only_on_the_tracers(case):
    c, sim = case, case.sim
    X1 = c.solve("per_tracer", rtol=1e-12)                       # flow bjacobi, follow
    assert X1[2] > 0 and relmax(X1[0], c.xs) < 1e-7
    sim.set_opts(pc_type="asm", asm_overlap=1)
    sim.set_aux_pc("bjacobi")
    got = c.solve("per_tracer", rtol=1e-12)                      # flow asm, tracers under block Jacobi
    assert same(got, X1), (got[2:], X1[2:])
    sim.set_aux_pc("follow")
    asm = c.solve("per_tracer", rtol=1e-12)                      # flow asm, follow: the tracers under asm
    print("its bjacobi", X1[3], "asm", asm[3], "asm against direct", relmax(asm[0], c.xs))
    assert asm[2] > 0 and not np.array_equal(asm[0], X1[0])
    assert relmax(asm[0], c.xs) < 1e-7
    # the mirror: flow bjacobi, tracers under asm overlap 1
    sim.set_opts(pc_type="bjacobi")
    sim.set_aux_pc("asm", 1, 0, "ilu")
    assert same(c.solve("per_tracer", rtol=1e-12), asm)
    # ILU(1) and sub-preconditioner lu of the tracers' own against their follow twins
    sim.set_aux_pc("follow")
    sim.set_opts(pc_type="bjacobi", ilu_levels=1)
    twin = c.solve("per_tracer", rtol=1e-12)
    sim.set_opts(pc_type="asm", ilu_levels=0)
    sim.set_aux_pc("bjacobi", 1, 1, "ilu")
    got = c.solve("per_tracer", rtol=1e-12)
    assert twin[2] > 0 and same(got, twin) and not np.array_equal(twin[0], X1[0])
    assert relmax(twin[0], c.xs) < 1e-7
    sim.set_aux_pc("follow")
    sim.set_opts(pc_type="bjacobi", ilu_levels=0)
    sim.set_sub_pc("lu")
    twin = c.solve("per_tracer", rtol=1e-12)
    sim.set_sub_pc("ilu")
    sim.set_aux_pc("bjacobi", 1, 0, "lu")
    got = c.solve("per_tracer", rtol=1e-12)
    print("sub lu its", twin[3])
    assert twin[2] > 0 and same(got, twin)
    assert relmax(twin[0], c.xs) < 1e-7
    reset(sim)
    assert same(c.solve("per_tracer", rtol=1e-12), X1)


def configure(sim, flow, aux):
    sim.set_opts(pc_type=flow.get("pc", "bjacobi"), asm_overlap=1, ilu_levels=0)
    sim.set_sub_pc(flow.get("sub", "ilu"))
    sim.set_aux_pc(aux.get("pc", "bjacobi"), 1, 0, aux.get("sub", "ilu"))


@pytest.mark.parametrize("flow,aux", [(dict(pc="asm"), dict(pc="bjacobi")), (dict(pc="bjacobi"), dict(pc="asm")),
                                      (dict(pc="bjacobi", sub="lu"), dict(pc="bjacobi", sub="ilu"))])
def test_a_tracer_solve_between_two_flow_steps_leaves_them_alone(flow, aux):
    """timestep, tracer solve, timestep against the same two steps without the tracer solve: the flow steps' reasons, counts
    and solutions bit for bit -- nothing of the tracers' factor, flags or work vectors is left for the flow solver"""
    runs = []
    for with_tracers in (False, True):
        c = Case("we", 2)
        sim = c.sim
        configure(sim, flow, aux)
        y = c.y.copy()
        steps = [sim.timestep(c.dt, c.dt, y)]
        y1 = y.copy()
        if with_tracers:
            X, new, reason, its = c.solve("per_tracer", rtol=1e-12)
            assert reason > 0 and its > 0
        steps.append(sim.timestep(2 * c.dt, c.dt, y))
        assert all(s[0] > 0 and s[2] > 0 for s in steps), steps
        runs.append((steps, y1, y.copy()))
        sim.destroy()
    print(flow, aux, "flow steps (reason, newton, krylov):", runs[0][0], runs[1][0])
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("eos,nt", [("we", 2), ("wce", 3)])
def test_coupled_under_the_reference_defaults_against_the_oracle(oracle, eos, nt):
    """flow asm, tracers block Jacobi, coupled, nt = np: the oracle's block GMRES(30) + block-Jacobi ILU(0) on the same
    system at rtol 1e-5 -- same reason, iteration count within one, same solution"""
    c = Case(eos, nt)
    osim = ol.OracleSim(oracle, c.lm, KIND[eos])
    V, b = c.block_system("beuler")
    oreason, xo, oits, hist = osim.ksp_solve(block_values(V).ravel(), b, ksp_type=1, restart=30, rtol=1e-5)
    c.sim.set_opts(pc_type="asm", asm_overlap=1)
    c.sim.set_aux_pc("bjacobi")
    s0 = c.sim.tracer_assembly_sweeps()
    X, new, reason, its = c.solve("coupled", rtol=1e-5)
    print(eos, "coupled its", its, "oracle its", oits, "reason", reason, oreason, "difference", np.abs(X - xo).max(), "of", np.abs(xo).max())
    assert c.sim.tracer_assembly_sweeps() - s0 == 1
    assert reason == oreason and reason > 0
    assert abs(its - oits) <= 1
    assert np.abs(X - xo).max() <= 1e-8 * np.abs(xo).max()
    assert c.sim.timestep(c.dt, c.dt, c.y)[0] > 0    # the flow solver under asm again
    c.sim.destroy(); osim.close()


def test_coupled_refuses_what_the_auxiliary_preconditioner_does_not_cover(case):
    """an explicit auxiliary asm, lu, ILU(1) or sub lu, and lgmres / bcgsl: -2, named, no assembly sweep, whatever the flow
    solver uses; none and bjacobi of the tracers' own run under a flow ILU(1), lu or sub lu"""
    from waiwera_amd.flow_simulation import WaiError
    c, sim = case, case.sim
    sim.set_tracer_solve_mode("coupled")
    sim.set_aux_solver("gmres", rtol=1e-12)

    def refused(word):
        s0 = sim.tracer_assembly_sweeps()
        with pytest.raises(WaiError) as e:
            sim.aux_solve("beuler", c.dt, 1.3, c.alx1, c.alx2, c.X0.copy(), np.zeros(c.n))
        assert "(-2)" in str(e.value) and word in str(e.value) and "coupled" in str(e.value), str(e.value)
        assert sim.tracer_assembly_sweeps() == s0
    for setting, word in ((("asm", 1, 0, "ilu"), "asm"), (("lu", 1, 0, "ilu"), "lu preconditioner"),
                          (("bjacobi", 1, 1, "ilu"), "ILU(k)"), (("bjacobi", 1, 0, "lu"), "WAI_SUB_LU")):
        sim.set_aux_pc(*setting)
        refused(word)
    sim.set_aux_pc("bjacobi")
    for ksp in ("lgmres", "bcgsl"):
        sim.set_aux_solver(ksp, rtol=1e-12)
        refused(ksp)
    for flow in (dict(pc_type="bjacobi", ilu_levels=1), dict(pc_type="lu", ilu_levels=0), dict(pc_type="asm", ilu_levels=0)):
        sim.set_opts(**flow)
        for pc in ("bjacobi", "none"):
            sim.set_aux_pc(pc)
            X, new, reason, its = c.solve("coupled", rtol=1e-12)
            assert reason > 0, (flow, pc, reason)
            if pc == "bjacobi":
                assert relmax(X, c.xs) < 1e-7, (flow, pc)
    sim.set_opts(pc_type="bjacobi", ilu_levels=0)
    sim.set_sub_pc("lu")
    sim.set_aux_pc("bjacobi", 1, 0, "ilu")
    X, new, reason, its = c.solve("coupled", rtol=1e-12)
    assert reason > 0 and relmax(X, c.xs) < 1e-7
    reset(sim)


@pytest.mark.parametrize("one_block", [False, True])
@pytest.mark.parametrize("ksp", ["lgmres", "bcgsl"])
def test_lgmres_and_bcgsl_per_tracer(ksp, one_block):
    """rtol 1e-12 against scipy's direct solve of each tracer's system, on the bricks and with one block per rank; the flow
    solver (BiCGStab on the same work vectors) runs as before afterwards"""
    c = Case("we", 2, one_block=one_block)
    V, b = c.block_system("beuler")
    xs = direct_solutions(c.rowptr, c.colidx, V, b)
    X, new, reason, its = c.solve("per_tracer", "beuler", ksp, rtol=1e-12)
    print(ksp, "one block" if one_block else "bricks", "its", its, "reason", reason, "against direct", relmax(X, xs))
    assert reason > 0
    assert relmax(X, xs) < 1e-7
    Al = np.zeros(c.n)
    c.sim.aux_lhs(0.0, None, Al)
    assert np.array_equal(new, Al * X)
    assert c.sim.timestep(c.dt, c.dt, c.y)[0] > 0
    c.sim.destroy()
