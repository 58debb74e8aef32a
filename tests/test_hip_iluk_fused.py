"""Block-Jacobi ILU(k), k > 0, applied in one fused launch: k_pc_wide's two-pattern form -- A x on the Jacobian's planes,
the two sweeps on the filled factor's own -- wherever every filled row of a brick has at most 16 blocks and every brick
at most 1024 rows (meshes of at most 8 blocks per row, one rank).

The shapes are the smallest of tests/test_hip_fused_operator.py's table at which the kernel can still go wrong; the filled
width of each is computed here on the CPU from the pattern (the level-of-fill rule of PETSc's MatILUFactorSymbolic,
restated below) and asserted: <= 16 for every case claimed as fused, > 16 for the case that must keep the
launch-per-level path.

Bars.  One application at a time against the long-double reference of tests/fused_reference.py, handed the filled pattern
with explicit zeros in the fill slots (ILU(k)'s numeric phase is ILU(0) on that pattern), with that file's bars: z within
1e-12 of max|z_ref|, an inner product within 1e-13 of sum |a_i b_i|, three identical applications bit-identical, slots a
phase does not write untouched.  Fused against the launch-per-level path on the same matrix (WAI_ILUK_LEVEL_PATH=1, the
path this replaces): 1e-10 of max|z|, the bar tests/test_hip_wide_mesh.py holds its applications to.  Whole solves against
the oracle's ILU(1) on the same subdomains: both converged for the same reason, iteration counts within one, solutions
within 1e-7 (what tests/test_hip_pc.py asks of two solves stopped at rtol 1e-10).

The fallback build (tools/ci_fallback_kernels.sh, WAI_FALLBACK_BUILD=1) replaces the narrow brick kernels only: wide
schedules keep k_pc_wide there, so the names expected here are the same in both builds."""
import heapq

import numpy as np
import pytest

from oracle import binding as ol
from tests import fused_reference as fr
from tests import test_hip_fused_operator as fo
from waiwera_amd.cases import make_case, scaled
from waiwera_amd.lib import WaiError

pytestmark = pytest.mark.gpu

KIND, BS = fo.KIND, fo.BS
LEVELS = "k_spmv + k_lvl_solve per level"

# id: (eos, dims, brick, ILU level)
CASES = {
    "we_ragged": ("we", (12, 10, 9), (4, 4, 2), 1),          # ragged in y and z, 45 bricks: not a multiple of 8
    "wce_ragged": ("wce", (13, 9, 5), (5, 4, 2), 1),         # ragged in x, y and z
    "w_bs1": ("w", (12, 10, 9), (4, 4, 4), 1),               # 1 x 1 blocks
    "wsce_bs4": ("wsce", (8, 8, 4), (4, 4, 4), 1),           # 4 x 4 blocks
    "we_bench_brick": ("we", (40, 36, 6), (16, 16, 2), 1),   # 512-row bricks beside ragged ones (LPT order)
    "we_ragged_ilu2": ("we", (12, 10, 9), (4, 4, 2), 2),     # ILU(2) in two-layer bricks: still <= 16 blocks per row
}
# ILU(2) in 4 x 4 x 4 bricks fills rows beyond 16 blocks: the launch-per-level path
TOO_WIDE = ("we", (12, 10, 9), (4, 4, 4), 2)


def iluk_pattern(rp, ci, sub, levels):
    """the pattern of block-Jacobi ILU(levels): per brick of sub, an entry created while row k is eliminated from row i
    gets lev(i, k) + lev(k, j) + 1, an entry reached twice keeps the smaller level, kept when <= levels.  Returns the
    filled BCSR pattern (couplings that leave a brick kept as they are: the operator's, not the factor's), for every
    entry the index of the original entry it holds (-1: fill), and the most in-brick blocks of any row."""
    n = len(rp) - 1
    owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
    upper = [None] * n          # per row: {j > i: level} of the filled row
    rows, width = [], 0
    for i in range(n):
        lo, hi = sub[owner[i]], sub[owner[i] + 1]
        lev = {int(ci[q]): 0 for q in range(rp[i], rp[i + 1]) if lo <= ci[q] < hi}
        heap = [j for j in lev if j < i]
        heapq.heapify(heap)
        done = set()
        while heap:
            k = heapq.heappop(heap)
            if k in done:
                continue
            done.add(k)
            for j, lkj in upper[k].items():
                lv = lev[k] + lkj + 1
                if lv > levels:
                    continue
                if j in lev:
                    lev[j] = min(lev[j], lv)
                else:
                    lev[j] = lv
                    if j < i:
                        heapq.heappush(heap, j)
        upper[i] = {j: l for j, l in lev.items() if j > i}
        width = max(width, len(lev))
        orig = {int(ci[q]): q for q in range(rp[i], rp[i + 1])}
        rows.append(sorted(set(lev) | set(orig)))
    rpf = np.zeros(n + 1, dtype=np.int64)
    rpf[1:] = np.cumsum([len(r) for r in rows])
    cif = np.array([j for r in rows for j in r], dtype=np.int64)
    src = np.full(cif.size, -1, dtype=np.int64)
    for i in range(n):
        orig = {int(ci[q]): q for q in range(rp[i], rp[i + 1])}
        for t, j in enumerate(rows[i]):
            src[rpf[i] + t] = orig.get(j, -1)
    return rpf, cif, src, width


def mesh_pattern(lm):
    """(rowptr, colidx) of the owned cells' block rows from the mesh's faces: the cell itself and its neighbours, ascending"""
    n = lm.n_owned
    fc = np.asarray(lm.face_cells)
    nb = [{i} for i in range(n)]
    for a, b in fc:
        if a < n and b < n:
            nb[a].add(int(b)); nb[b].add(int(a))
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(s) for s in nb])
    return rp, np.array([j for s in nb for j in sorted(s)], dtype=np.int64)


class FilledRef:
    """the long-double reference handed the filled pattern: fill slots start at zero, A x on the matrix's own pattern"""

    def __init__(self, rp, ci, val, bs, sub, fill):
        rpf, cif, src, _ = fill
        V = np.asarray(val).reshape(-1, bs, bs)
        Vf = np.zeros((cif.size, bs, bs))
        Vf[src >= 0] = V[src[src >= 0]]
        self.ilu = fr.BlockILU0(rpf, cif, Vf.ravel(), bs, sub)
        self.rp, self.ci, self.bs = rp, ci, bs

    def solve(self, r):
        return self.ilu.solve(r)

    def operator(self, val, x):
        return self.ilu.solve(fr.spmv(self.rp, self.ci, val, self.bs, x))


class FilledChecker(fo.Checker):
    def __init__(self, sim, rp, ci, sub, bs, val, label, fill):
        self.sim, self.bs, self.val, self.label = sim, bs, val, label
        sim.set_jacobian_values(val)
        assert sim.pc_setup() == 0
        self.ref = FilledRef(rp, ci, val, bs, sub, fill)
        n = len(rp) - 1
        rng = np.random.default_rng(11)
        self.x, self.x2, self.aux = (fr.spread_vector(n, bs, rng) for _ in range(3))
        s = np.zeros(16)
        s[fr.S_RHO], s[fr.S_RHOOLD], s[fr.S_OMEGA], s[fr.S_BETA] = 0.83, 1.7, 0.61, 2.3
        s[fr.S_D1:fr.S_W2 + 1] = rng.normal(size=5)
        s[10:15] = rng.normal(size=5)
        s[fr.S_ALPHA] = fo.ALPHA
        self.scal_in = s
        self.rows = {}


_systems = {}


def system(oracle, key):
    """mesh, FD Jacobian of the case's state, right-hand side and the filled pattern: computed once per shape and shared
    (nothing here is modified by a test)"""
    eos, dims, brick, levels = key
    if key not in _systems:
        g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=(eos == "we"))
        osim = ol.OracleSim(oracle, lm, KIND[eos])
        osim.set_regions(region)
        yo = osim.yvec(scaled(prim, region, eos).ravel().copy())
        assert osim.pre_eval(yo) == 0
        L = osim.lhs()
        err, f = osim.residual(yo, 5.0e4, L)
        err, J = osim.jacobian(yo, 5.0e4, L, f, mode=0)
        assert err == 0
        rp, ci = osim.pattern()
        osim.close()
        fill = iluk_pattern(rp, ci, np.asarray(lm.sub_ptr), levels)
        _systems[key] = dict(lm=lm, prim=prim, region=region, rp=rp, ci=ci, J=J, f=f, fill=fill)
    return _systems[key]


def fused_name(bs, levels):
    return "k_pc_wide<%d,spmv> on the filled factor (block Jacobi, ILU(%d))" % (bs, levels)


def make_sim(S, eos, levels, **opts):
    from waiwera_amd.flow_simulation import FlowSimulation
    sim = FlowSimulation(S["lm"], eos=eos)
    sim.set_regions(S["region"])
    sim.set_opts(pc_type="bjacobi", ilu_levels=levels, **opts)
    sim.set_jacobian_values(S["J"])
    return sim


def relmax(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("case", list(CASES))
def test_filled_width_fits_the_wide_descriptor(case):
    """the condition of the fused path, on the CPU: no filled row of any brick has more than 16 blocks, no brick more than
    1024 rows (and the fill is real: wider than the mesh's own rows)"""
    eos, dims, brick, levels = CASES[case]
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=(eos == "we"))
    rp, ci = mesh_pattern(lm)
    sub = np.asarray(lm.sub_ptr)
    width = iluk_pattern(rp, ci, sub, levels)[3]
    owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
    inside = np.zeros(lm.n_owned, dtype=int)
    np.add.at(inside, np.repeat(np.arange(lm.n_owned), np.diff(rp)), owner[ci] == np.repeat(owner, np.diff(rp)))
    print(case, "filled width", width, "ILU(0) width", inside.max())
    assert inside.max() < width <= 16 and np.diff(sub).max() <= 1024


def test_too_wide_case_is_too_wide():
    eos, dims, brick, levels = TOO_WIDE
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=True)
    rp, ci = mesh_pattern(lm)
    assert iluk_pattern(rp, ci, np.asarray(lm.sub_ptr), levels)[3] > 16


@pytest.mark.parametrize("case", list(CASES))
def test_routing(oracle, case):
    """pc_kernel_name() names k_pc_wide and the ILU level; ILU(0) on the same context keeps the kernel it had"""
    eos, dims, brick, levels = CASES[case]
    S = system(oracle, CASES[case])
    assert S["fill"][3] <= 16
    sim = make_sim(S, eos, levels)
    assert sim.pc_setup() == 0
    name = sim.pc_kernel_name()
    assert name == fused_name(BS[eos], levels) and "k_pc_wide" in name and "ILU(%d)" % levels in name, name
    assert not sim.pc_axpy_capable()          # no composed operand: BiCGStab takes the four-launch form
    sim.set_opts(ilu_levels=0)
    assert sim.pc_setup() == 0
    assert "wide" not in sim.pc_kernel_name() and "ILU(" not in sim.pc_kernel_name(), sim.pc_kernel_name()
    sim.destroy()


def test_routing_keeps_the_level_path_where_the_fill_is_wider(oracle, monkeypatch):
    """fill beyond 16 blocks per row, a brick of more than 1024 rows, and the switch that keeps the level path"""
    eos, dims, brick, levels = TOO_WIDE
    S = system(oracle, TOO_WIDE)
    assert S["fill"][3] > 16
    sim = make_sim(S, eos, levels)
    assert sim.pc_setup() == 0
    name = sim.pc_kernel_name()
    assert LEVELS in name and "ILU(2)" in name and "k_pc_wide" not in name, name
    # the same mesh with ILU(1): 13 blocks, fused
    sim.set_opts(ilu_levels=1)
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(2, 1), sim.pc_kernel_name()
    monkeypatch.setenv("WAI_ILUK_LEVEL_PATH", "1")
    assert sim.pc_setup() == 0
    name = sim.pc_kernel_name()
    assert LEVELS in name and "ILU(1)" in name, name
    sim.destroy()
    monkeypatch.delenv("WAI_ILUK_LEVEL_PATH")
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(16, 16, 10), brick=(16, 16, 5), eos="we", lens=True)
    assert np.diff(lm.sub_ptr).max() == 1280
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    sim.set_opts(pc_type="bjacobi", ilu_levels=1)
    y = scaled(prim, region, "we").ravel().copy()
    L = np.zeros(sim.num_dof)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, 1.0, y, L)
    assert sim.jacobian(0.0, 5.0e4, y, L) == 0
    assert sim.pc_setup() == 0
    name = sim.pc_kernel_name()
    assert LEVELS in name and "ILU(1)" in name, name
    sim.destroy()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", list(CASES))
def test_one_application_against_long_double_reference(oracle, case):
    """z = B^-1 A x and z = B^-1 x, dot modes 0 - 4, the reductions finished in the launch and by k_finalize, on the FD
    Jacobian and on random O(1) values; what the kernel cannot serve (a composed operand, the interior / face split) is
    refused, not answered"""
    eos, dims, brick, levels = CASES[case]
    bs = BS[eos]
    S = system(oracle, CASES[case])
    rp, ci, sub = S["rp"], S["ci"], np.asarray(S["lm"].sub_ptr)
    assert S["fill"][3] <= 16
    sim = make_sim(S, eos, levels)
    rps, cis = sim.setup_jacobian()
    assert np.array_equal(rp, rps) and np.array_equal(ci, cis)
    for values in ("fd", "random"):
        val = S["J"] if values == "fd" else fr.random_values(rp, ci, bs, np.random.default_rng(12))
        ck = FilledChecker(sim, rp, ci, sub, bs, val, (case, values), S["fill"])
        kernel = sim.pc_kernel_name()
        assert kernel == fused_name(bs, levels), kernel
        with pytest.raises(WaiError):
            ck.apply(x2=ck.x2)
        with pytest.raises(WaiError):
            ck.apply(x2=ck.x2, spmv=False)
        with pytest.raises(WaiError):
            ck.apply(split=True)
        for tag, spmv in (("B^-1 x", False), ("B^-1 A x", True)):
            ck.variant(tag, spmv, False, False)
        ck.local_input(sub, rp, ci)
        ck.report(kernel)
    sim.destroy()


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_launch_per_level_path(oracle, case, monkeypatch):
    """the same matrix factored and applied by the path this replaces (k_lvl_factor / k_spmv + k_lvl_solve per level on
    the same filled pattern): applications within 1e-10; wai_bench_kernel 23 runs that path on the fused schedule's factor"""
    eos, dims, brick, levels = CASES[case]
    S = system(oracle, CASES[case])
    n = len(S["rp"]) - 1
    sim = make_sim(S, eos, levels)
    rng = np.random.default_rng(5)
    r, x = rng.normal(size=n * BS[eos]), fr.spread_vector(n, BS[eos], rng)
    out = {}
    for path in ("fused", "levels"):
        if path == "levels":
            monkeypatch.setenv("WAI_ILUK_LEVEL_PATH", "1")
        assert sim.pc_setup() == 0
        name = sim.pc_kernel_name()
        assert ("k_pc_wide" in name) == (path == "fused") and (LEVELS in name) == (path == "levels"), (path, name)
        z = np.zeros(n * BS[eos])
        sim.pc_apply(r, z)
        out[path] = (z, sim.pc_operator(x, spmv=True)[0])
    monkeypatch.delenv("WAI_ILUK_LEVEL_PATH")
    for a, b in zip(out["fused"], out["levels"]):
        print(case, "fused against levels", relmax(a, b))
        assert relmax(a, b) < 1e-10
    assert sim.pc_setup() == 0 and "k_pc_wide" in sim.pc_kernel_name()
    assert sim.bench_kernel(23, reps=2) > 0.0 and sim.bench_kernel(2, reps=2) > 0.0
    # the probe leaves the context as it was: the same application again, bit for bit
    z = np.zeros(n * BS[eos])
    sim.pc_apply(r, z)
    assert np.array_equal(z, out["fused"][0])
    sim.destroy()


@pytest.mark.parametrize("case", ["we_ragged", "wce_ragged"])
@pytest.mark.parametrize("ksp,kt", [("bcgs", 0), ("gmres", 1)])
def test_whole_solves_against_the_oracle(oracle, case, ksp, kt):
    """BiCGStab and GMRES with fused ILU(1) at rtol 1e-10 against the oracle's solves with ILU(1) on the same subdomains"""
    eos, dims, brick, levels = CASES[case]
    S = system(oracle, CASES[case])
    n = len(S["rp"]) - 1
    sim = make_sim(S, eos, levels, ksp_type=ksp, ksp_rtol=1e-10)
    osim = ol.OracleSim(oracle, S["lm"], KIND[eos])
    osim.set_regions(S["region"])
    osim.set_asm(0)
    osim.set_ilu_levels(levels)
    assert sim.pc_setup() == 0 and osim.pc_setup(S["J"]) == 0
    assert sim.pc_kernel_name() == fused_name(BS[eos], levels)
    x = np.zeros(n * BS[eos])
    its, reason, rn = sim.ksp_solve(S["f"], x)
    oreason, xo, oits, hist = osim.ksp_solve(S["J"], S["f"], ksp_type=kt, rtol=1e-10)
    print(case, ksp, "its", its, oits, "reason", reason, oreason, "x", relmax(x, xo[:x.size]))
    assert reason > 0 and reason == oreason, (reason, oreason)
    assert abs(its - oits) <= 1, (its, oits)
    assert relmax(x, xo[:x.size]) < 1e-7
    sim.destroy(); osim.close()


def test_timestep_against_the_level_path():
    """one backward-Euler step with ilu_levels = 1 on 512-row bricks (the fused launch) against the same step on 1280-row
    bricks (the launch-per-level path).  The two preconditioners differ, so both solve to ksp_rtol 1e-12: the Newton
    iterates then do not depend on the preconditioner -- same Newton count, solution within 1e-9 relative"""
    from waiwera_amd.flow_simulation import FlowSimulation
    res = {}
    for tag, brick in (("fused", (16, 16, 2)), ("levels", (16, 16, 5))):
        g, lm, prim, region = make_case(dims=(16, 16, 10), brick=brick, eos="we", lens=True)
        sim = FlowSimulation(lm, eos="we")
        sim.set_regions(region)
        sim.set_opts(pc_type="bjacobi", ilu_levels=1, ksp_rtol=1e-12, ftol_rel=1e-9)
        y = scaled(prim, region, "we").ravel().copy()
        reason, nits, kits = sim.timestep(0.0, 1.0e4, y)
        name = sim.pc_kernel_name()
        assert reason > 0 and ("k_pc_wide" in name) == (tag == "fused") and "ILU(1)" in name, (tag, reason, name)
        assert (np.diff(lm.sub_ptr).max() > 1024) == (tag == "levels")
        ijk = np.asarray(lm.owned_ijk)          # the bricks order the cells: compare in the grid's own order
        order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))
        res[tag] = (nits, y.reshape(-1, 2)[order], kits)
        sim.destroy()
    print("timestep: Newton", res["fused"][0], res["levels"][0], "Krylov", res["fused"][2], res["levels"][2])
    assert res["fused"][0] == res["levels"][0]
    yf, yl = res["fused"][1], res["levels"][1]
    err = np.abs(yf - yl).max(axis=0) / np.abs(yl).max(axis=0)
    print("timestep: fused against levels", err)
    assert err.max() < 1e-9, err


def test_bicgstab_iteration_is_four_launches(oracle):
    """one BiCGStab iteration under fused ILU(1): fused A P, S = R - alpha V, fused A S, the X / R / P update -- four
    launches by the library's counter (+ the solve's set-up and the speculative half iteration that is thrown away)"""
    eos, dims, brick, levels = CASES["we_ragged"]
    S = system(oracle, CASES["we_ragged"])
    n = len(S["rp"]) - 1
    sim = make_sim(S, eos, levels, ksp_type="bcgs", ksp_rtol=1e-10)
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(2, 1)
    x = np.zeros(n * 2)
    k0, c0 = sim.launch_stats()
    its, reason, rn = sim.ksp_solve(S["f"], x)
    k1, c1 = sim.launch_stats()
    assert reason > 0 and its >= 5
    assert 4 * its <= k1 - k0 <= 4 * its + 8, (its, k1 - k0)
    sim.destroy()
