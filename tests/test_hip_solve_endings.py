"""How linear solves END on the device: a singular pivot on every factorisation path (-11), the iteration cap (-3), the
tolerances (2, 3), a zero right-hand side, a system solved in one step, breakdown (-5), NaN (-9) -- through wai_pc_setup,
wai_pc_apply, wai_ksp_solve, wai_newton_step and wai_timestep -- and what the next solve on the same context sees of the one
that ended.  The constructions and the long-double restatements are tests/solve_endings_reference.py's, pinned on the CPU
by tests/test_solve_endings_reference.py.

Bounds.  Bit-for-bit comparisons are against the device's own fresh context on the same matrix (determinism).  x and rnorm
after k <= 5 iterations are held to the long-double restatement within TEN TIMES the distance between the restatement's
double-precision and long-double runs on the same system (se.double_distance, evaluated again here on the CPU; the factor
for the device's other summation order).  MEASURED on the CPU, worst over the k of each row, relative (x to max |x|):

    system        BiCGStab merged     BiCGStab petsc      GMRES(30) k=1,2,3   GMRES(2) k=2,3,5
                  x        rnorm      x        rnorm      x        rnorm      x        rnorm
    w   bjacobi   4.6e-16  1.3e-14    4.6e-16  1.1e-15    6.4e-16  4.9e-16    6.4e-16  3.5e-13
    w   none      2.0e-16  5.8e-14    1.7e-16  1.8e-14    6.5e-16  1.2e-15    6.5e-16  9.0e-15
    we  bjacobi   3.8e-16  5.9e-14    3.6e-16  2.1e-14    5.4e-16  5.1e-16    4.6e-16  7.6e-13
    we  none      2.4e-16  3.2e-15    2.9e-16  4.4e-16    3.2e-16  2.1e-16    3.1e-16  1.2e-14
    wce bjacobi   3.4e-16  4.7e-13    3.4e-16  1.5e-13    2.3e-16  7.5e-16    3.2e-16  2.7e-12
    wce none      1.9e-16  2.2e-14    1.9e-16  4.0e-15    3.1e-16  4.1e-16    3.1e-16  7.7e-14
    wsce bjacobi  5.0e-16  5.1e-14    5.0e-16  4.7e-15    4.2e-16  8.6e-16    4.2e-16  4.5e-12
    wsce none     1.9e-16  4.8e-14    1.9e-16  1.2e-14    6.2e-16  2.4e-16    5.3e-16  6.9e-14

("merged": the residual norm derived from (S,S), (S,T), (T,T) as every launch form but WAI_BCGS=petsc does; the
restatement states both.  The double-precision run's inner products are numpy's, so a distance near 2e-16 -- one rounding
of a double -- is a property of the host's numpy as well.)  All are far below the 1e-10 beyond which a system would be too ill-conditioned for this.
LGMRES, BiCGStab(2) and rnorm against the true residual are held to the oracle with tests/test_hip_pc.py's tolerances
(x 1e-8 for BiCGStab(2), 1e-7 for LGMRES; the gap of rnorm within 10 x max(the oracle's gap, 2^-53) as
tests/test_hip_krylov_vec.py holds GMRES's estimate).

MEASURED on the device (MI355X; the tests print every figure before they assert): against the restatement the worst x
is 0.21 of its bound (wce bjacobi, GMRES k = 2: 4.8e-16 of 2.3e-15) and the worst rnorm 0.58 of its bound (wsce none,
GMRES k = 3: 1.4e-15 of 2.4e-15); every launch form but petsc returns the same bits.  Against the oracle: LGMRES
x 3.7e-16, rnorm 1.1e-14; BiCGStab(2) x 8.9e-15, rnorm 3.0e-10 (wsce, k = 4: a norm of 1e-8 |B^-1 b| that the sweep's
cancellation leaves to so many digits).  The gap of rnorm to the true residual: at most 0.18 of its
bound (2.0e-16 of |B^-1 b|).  On the skew chain BiCGStab ends with -5 at its 1 in every form (rnorm 0.0, NaN in the petsc
form: not asserted, alpha is rho / 0 there), BiCGStab(2) with -5 at its 0 like the oracle, GMRES(30) and LGMRES with -3 at
the cap of 40 like the restatement and the oracle (5.385164807134504 and 8.0).  BiCGStab(2) on the one-step system: -5 at
its 0 with x = A^-1 b, like the oracle.

Before the fixes of this change (the library of the parent commit): every path's wai_pc_setup returned 1 -- all eleven
flags work -- and then the first wai_ksp_solve iterated on the factor of 1 / 0 and ended with -9 and rnorm NaN, because
do_pc_setup had recorded the system as the factor's owner before it read the flags; under pc_type lu, whose branch did not,
the reason was -11 but x came back as the never-written work vector.  Everything else here passed unchanged.

Left out, with the reason:
- the tracer systems' factor kernels (k_dg_*): no entry point prescribes their matrix;
- near-singular pivots: the library, like block_inverse, flags exact zeros only;
- divergence (-4, BiCGStab alone: GMRES's estimate never grows).  The CPU search with the long-double restatement --
  about 26 000 tridiagonal pc-none systems of 64 unknowns (constant, periodic, alternating-sign and power-of-two diagonals,
  sub- and super-diagonals from -4 to 16, four right-hand sides), up to 40 iterations each -- found no system whose
  residual passes 1e4 |b| by a factor 10 at an iteration where nothing else fires and on which the double and long-double
  runs, in both forms of the norm, agree on the iteration.  The fourteen that reached -4 at all did so through a
  near-breakdown (a jump of 1e4 to 1e15 in one iteration) whose size rounding decides.  No case is pinned.
- pc_type lu on several ranks: lu_setup's "1" is decided per rank on the host, not collectively (the two-rank case here
  runs block Jacobi, whose flags are collective)."""
import os

import numpy as np
import pytest

from oracle import binding as ol
from tests import fused_reference as fr
from tests import solve_endings_reference as se
from waiwera_amd.cases import make_case, scaled

pytestmark = pytest.mark.gpu

KIND = {"w": 0, "we": 1, "wce": 2, "wsce": 5}
BS = se.BS
LD = se.LD
LEVELS = "k_spmv + k_lvl_solve per level"
DRIVERS = ("bcgs", "gmres", "lgmres", "bcgsl")
OTYPE = {"bcgs": 0, "gmres": 1, "bcgsl": 2, "lgmres": 3}
OTOL = {"bcgsl": 1e-8, "lgmres": 1e-7}      # tests/test_hip_pc.py: test_bcgsl, test_lgmres
# the launch forms test_bicgstab_with_merged_reductions and test_bicgstab_fused_iteration switch between
BCGS_FORMS = {"default": {}, "fused": {"WAI_BCGS": "fused", "WAI_BCGS_COMPOSE": "0"}, "merged": {"WAI_BCGS": "merged"},
              "merged_env": {"WAI_BCGS_MERGED": "1"}, "composed": {"WAI_BCGS": "fused", "WAI_BCGS_COMPOSE": "1"},
              "fin_separate": {"WAI_BCGS": "fused", "WAI_FIN_SEPARATE": "1"}, "petsc": {"WAI_BCGS": "petsc"}}
FORM_KEYS = ("WAI_BCGS", "WAI_BCGS_COMPOSE", "WAI_FIN_SEPARATE", "WAI_BCGS_MERGED")


def new_sim(lm, eos, **opts):
    from waiwera_amd.flow_simulation import FlowSimulation
    sim = FlowSimulation(lm, eos=eos)
    if opts:
        sim.set_opts(**opts)
    return sim


def solve(sim, b, fill=7.0):
    """(its, reason, rnorm, x) with x pre-filled: whatever comes back was written by the solve"""
    x = np.full(b.size, fill)
    its, reason, rn = sim.ksp_solve(b, x)
    return its, reason, rn, x


def same(a, b):
    return a[:3] == b[:3] and np.array_equal(a[3], b[3])


def set_form(monkeypatch, form):
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in BCGS_FORMS[form].items():
        monkeypatch.setenv(k, v)


# ---- a. a singular pivot on every factorisation path ------------------------------------------------------------------------
def box_mesh(eos, dims, brick, one_block=False):
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=False)
    return lm, one_block


def triangle(eos):
    return fr.triangle_mesh(eos)[1], False


def wide(eos):
    from tests import wide_mesh as wm
    return wm.wide_case(eos)[0], False


# id: (eos, mesh, settings, what pc_kernel_name() must say, zero the whole row)
#  settings: opts for wai_set_opts, "sub" for wai_set_sub_pc, "order" for wai_set_pc_ordering, "env" at the set-up
PATHS = {
    # the DILU pivots of the brick kernels: k_dilu_pivots<1 / 2 / 4> and, for 3 x 3 blocks, k_dilu_pivots_lds with the
    # couplings in registers (one wave per brick) and staged in LDS (128-row bricks)
    "dilu_generic_w": ("w", lambda: box_mesh("w", (8, 8, 4), (4, 4, 4)), {}, lambda s: s.startswith("k_pc<1,spmv,dilu-scaled"), False),
    "dilu_park_we": ("we", lambda: box_mesh("we", (8, 8, 4), (4, 4, 2)), {}, lambda s: s == "k_pc_park<spmv,col16>", False),
    "dilu_wave_wce": ("wce", lambda: box_mesh("wce", (8, 8, 4), (4, 4, 2)), {}, lambda s: s == "k_pc_wave<3,spmv>", False),
    "dilu_rows_wce": ("wce", lambda: box_mesh("wce", (8, 8, 8), (8, 4, 4)), {}, lambda s: s.startswith("k_pc_rows<3,spmv"), False),
    "dilu_rows_wsce": ("wsce", lambda: box_mesh("wsce", (8, 8, 4), (4, 2, 2)), {}, lambda s: s.startswith("k_pc_rows<4,spmv"), False),
}
# the paths that serve every block size, each with all four: the stored factor (k_ilu_factor: a cell graph with triangles), the
# wide factor (k_ilu_factor_wide: rows of up to 15 blocks), the level path (k_lvl_factor: one block per rank, 1280 rows),
# PCASM's extended factor fused and by the launches it replaces, ILU(1), the multicolour ordering (k_colour_factor),
# sub-preconditioner lu (pc_lu.hip.h) and pc_type lu (the host's dense inverses)
ASM_NAME = "on the extended system (ASM, ILU(0))"
for _eos in ("w", "we", "wce", "wsce"):
    _b = (4, 4, 4) if _eos == "w" else (4, 2, 2) if _eos == "wsce" else (4, 4, 2)
    _more = {
        "stored_" + _eos: (lambda e=_eos: triangle(e), {}, lambda s, e=_eos: s.startswith("k_pc<%d,spmv,ilu," % BS[e]), False),
        "wide_" + _eos: (lambda e=_eos: wide(e), {}, lambda s, e=_eos: s == "k_pc_wide<%d,spmv>" % BS[e], False),
        "level_" + _eos: (lambda e=_eos: box_mesh(e, (16, 16, 5), (16, 16, 5), True), {}, lambda s: s == LEVELS, False),
        "asm_" + _eos: (lambda e=_eos, b=_b: box_mesh(e, (8, 8, 4), b), {"opts": {"pc_type": "asm"}},
                        lambda s, e=_eos: s.startswith("k_pc_wide<%d,spmv,map>" % BS[e]) and ASM_NAME in s, True),
        "asm_unfused_" + _eos: (lambda e=_eos, b=_b: box_mesh(e, (8, 8, 4), b), {"opts": {"pc_type": "asm"}, "env": {"WAI_ASM_UNFUSED": "1"}},
                                lambda s: s.startswith("k_spmv + ") and ASM_NAME in s and "map" not in s, True),
        "ilu1_" + _eos: (lambda e=_eos, b=_b: box_mesh(e, (8, 8, 4), b), {"opts": {"ilu_levels": 1}}, lambda s: "ILU(1)" in s, False),
        "colour_" + _eos: (lambda e=_eos: box_mesh(e, (6, 6, 4), (3, 3, 2)), {"order": "multicolour"},
                           lambda s, e=_eos: s == "k_pc_colour<%d,spmv>" % BS[e], True),
        "sublu_" + _eos: (lambda e=_eos: box_mesh(e, (6, 6, 4), (3, 3, 2)), {"sub": "lu"},
                          lambda s: "k_sublu_solve" in s and "block Jacobi" in s, False),
        "lu_" + _eos: (lambda e=_eos: box_mesh(e, (6, 4, 4), (3, 2, 2)), {"opts": {"pc_type": "lu"}}, lambda s: "k_lu_apply" in s, True),
    }
    for _id, _rest in _more.items():
        PATHS[_id] = (_eos,) + _rest


def path_sim(path, monkeypatch):
    eos, mesh, settings, name_ok, whole_row = PATHS[path]
    lm, one_block = mesh()
    if one_block:
        lm.sub_ptr = None
    for k, v in settings.get("env", {}).items():
        monkeypatch.setenv(k, v)
    sim = new_sim(lm, eos, ksp_rtol=1e-10, **settings.get("opts", {}))
    if one_block:
        lm.sub_ptr = np.array([0, lm.n_owned], dtype=np.int32)
    if "sub" in settings:
        sim.set_sub_pc(settings["sub"])
    if "order" in settings:
        sim.set_pc_ordering(settings["order"])
    return lm, sim


@pytest.mark.parametrize("path", list(PATHS))
def test_singular_pivot_on_every_factorisation_path(path, monkeypatch):
    """SINGULAR[bs] as the pivot of the first row of the first subdomain, a middle row of a middle one, the last row of
    the last: wai_pc_setup 1; wai_ksp_solve -11 with its 0, rnorm 0 and x zero -- twice, no new values in between, so the
    failed factor must not count as set up --; wai_pc_apply 1 with z untouched; and with the sound matrix back the solve of a
    fresh context, bit for bit"""
    eos, _, _, name_ok, whole_row = PATHS[path]
    bs = BS[eos]
    lm, sim = path_sim(path, monkeypatch)
    rp, ci = sim.setup_jacobian()
    assert np.array_equal(rp, se.mesh_pattern(lm)[0]) and np.array_equal(ci, se.mesh_pattern(lm)[1])
    n = sim.num_dof
    sub = np.asarray(lm.sub_ptr)
    val = se.diag_dominant_values(rp, ci, bs)
    b = np.random.default_rng(7).normal(size=n)
    r = np.random.default_rng(8).normal(size=n)
    # the fresh context's solve and application of the sound matrix
    fresh = path_sim(path, monkeypatch)[1]
    fresh.set_jacobian_values(val)
    assert fresh.pc_setup() == 0
    assert name_ok(fresh.pc_kernel_name()), fresh.pc_kernel_name()
    want = solve(fresh, b)
    zwant = np.zeros(n)
    assert fresh.pc_apply(r, zwant) == 0
    fresh.destroy()
    assert want[1] == 2, want[:3]
    mid = (len(sub) - 1) // 2
    for row in (int(sub[0]), int(sub[mid] + sub[mid + 1]) // 2, int(sub[-1]) - 1):
        sim.set_jacobian_values(se.singular_at(val, rp, ci, row, bs, whole_row=whole_row))
        assert sim.pc_setup() == 1, (path, row)
        assert name_ok(sim.pc_kernel_name()), sim.pc_kernel_name()
        for again in range(2):
            its, reason, rn, x = solve(sim, b)
            assert (reason, its, rn) == (-11, 0, 0.0), (path, row, again, reason, its, rn)
            assert not x.any(), (path, row, again, np.abs(x).max())
        z = np.full(n, 3.0)
        assert sim.pc_apply(r, z) == 1 and np.all(z == 3.0), (path, row)
        assert sim.pc_setup() == 1, (path, row)           # and once more: still reported
        sim.set_jacobian_values(val)
        assert sim.pc_setup() == 0, (path, row)
        got = solve(sim, b)
        assert same(got, want), (path, row, got[:3], want[:3])
        z = np.zeros(n)
        assert sim.pc_apply(r, z) == 0 and np.array_equal(z, zwant), (path, row)
    sim.destroy()


def test_a_failed_pivot_without_an_explicit_setup(monkeypatch):
    """the solve and the application make the set-up themselves: the first wai_ksp_solve on singular values is -11, and so
    is the second; wai_pc_apply first is 1 and the solve after it -11"""
    lm, sim = path_sim("dilu_park_we", monkeypatch)
    rp, ci = sim.setup_jacobian()
    n = sim.num_dof
    val = se.diag_dominant_values(rp, ci, 2)
    b = np.random.default_rng(7).normal(size=n)
    sv = se.singular_at(val, rp, ci, lm.n_owned // 2, 2)
    sim.set_jacobian_values(sv)
    for again in range(2):
        its, reason, rn, x = solve(sim, b)
        assert (reason, its, rn) == (-11, 0, 0.0) and not x.any(), (again, reason, its, rn)
    sim.set_jacobian_values(sv)
    z = np.full(n, 3.0)
    assert sim.pc_apply(b, z) == 1 and np.all(z == 3.0)
    assert solve(sim, b)[:3] == (0, -11, 0.0)
    sim.destroy()


# ---- b. a singular pivot from physics, through the Newton step ------------------------------------------------------------------
def dead_cell_case(eos):
    """a 4 x 4 x 4 box with one interior cell that holds no source, its porosity and permeabilities zero"""
    g, lm, prim, region = make_case(dims=(4, 4, 4), brick=(2, 2, 2), eos=eos, lens=False)
    ijk = np.asarray(lm.owned_ijk)
    srcs = set(int(c) for c in np.asarray(lm.src_cell)) if lm.n_src else set()
    dead = [q for q, (a, b, c) in enumerate(ijk) if 0 < a < 3 and 0 < b < 3 and 0 < c < 3 and q not in srcs][0]
    sound = lm.rock[dead].copy()
    lm.rock[dead, 0:3] = 0.0
    lm.rock[dead, 5] = 0.0
    return lm, prim, region, dead, sound


@pytest.mark.parametrize("eos", ["w", "we"])
def test_singular_pivot_from_physics_through_the_newton_step(oracle, eos):
    """A cell of zero porosity and zero permeability holds no mass and exchanges none: its mass-balance row of the FD
    Jacobian is exactly zero (the oracle's Jacobian is checked first: no NaN anywhere, the diagonal block exactly singular
    by block_inverse's arithmetic -- for eos we it is the block's first ROW that vanishes, the energy row keeps the rock's
    heat capacity; nothing about the rock had to be chosen beyond the two zeros).  The Newton step must report the failed
    linear solve and leave y alone; the time step must restore y and the regions; and the same context, given the sound rock,
    must step like a fresh one."""
    bs, dt = BS[eos], 1.0e4
    lm, prim, region, dead, sound = dead_cell_case(eos)
    osim = ol.OracleSim(oracle, lm, KIND[eos])
    osim.set_regions(region)
    y0 = scaled(prim, region, eos).ravel().copy()
    yo = osim.yvec(y0)
    assert osim.pre_eval(yo) == 0
    L = osim.lhs()
    err, f = osim.residual(yo, dt, L)
    err, J = osim.jacobian(yo, dt, L, f, mode=0)
    rp, ci = osim.pattern()
    osim.close()
    assert err == 0 and not np.isnan(J).any() and not np.isnan(f).any()
    dq = [q for q in range(rp[dead], rp[dead + 1]) if ci[q] == dead][0]
    block = J.reshape(-1, bs, bs)[dq]
    assert not se.block_inverse(block)[1] and not block[0].any(), block
    sim = new_sim(lm, eos)
    sim.set_regions(region)
    n = sim.num_dof
    # the Newton step: pre_eval and residual as a host makes them, then one device-resident iteration
    y = y0.copy()
    assert sim.pre_eval(0.0, y) == 0
    Ld, fd = np.zeros(n), np.zeros(n)
    sim.lhs(0.0, 0.0, y, Ld)
    assert sim.residual(0.0, dt, y, Ld, fd) == 0
    reason, kits, mr = sim.newton_step(0.0, dt, 0, y, Ld, fd)
    assert (reason, kits) == (-3, 0), (reason, kits)
    assert np.array_equal(y, y0)
    Jd = sim.jacobian_values().reshape(-1, bs, bs)
    assert not np.isnan(Jd).any() and not se.block_inverse(Jd[dq])[1], Jd[dq]
    # the time step: rejected, y and the regions as they were
    r0 = sim.regions().copy()
    treason, nits, kits = sim.timestep(0.0, dt, y)
    assert treason < 0 and np.array_equal(y, y0) and np.array_equal(sim.regions(), r0), (treason, nits, kits)
    # the sound rock: like a fresh context
    sim.update_rock(5, [dead], sound[5])
    for k in range(3):
        sim.update_rock(k, [dead], sound[k])
    got = sim.timestep(0.0, dt, y)
    lm2, prim2, region2, dead2, sound2 = dead_cell_case(eos)
    lm2.rock[dead2] = sound2
    fresh = new_sim(lm2, eos)
    fresh.set_regions(region2)
    y2 = y0.copy()
    want = fresh.timestep(0.0, dt, y2)
    assert got == want and got[0] > 0, (got, want)
    assert np.array_equal(y, y2) and np.array_equal(sim.regions(), fresh.regions())
    sim.destroy(); fresh.destroy()


# ---- c - h on the pinned systems -------------------------------------------------------------------------------------------------
SYSTEMS = [(eos, pc) for eos in ("w", "we", "wce", "wsce") for pc in ("bjacobi", "none")]
BRICK_KERNEL = {"w": "k_pc<1,spmv,dilu-scaled", "we": "k_pc_park<spmv,col16>", "wce": "k_pc_wave<3,spmv>", "wsce": "k_pc_rows<4,spmv"}


def pinned_sim(eos, pc, **opts):
    d = se.dominant(eos, pc)
    sim = new_sim(d["lm"], eos, pc_type=pc, **opts)
    rp, ci = sim.setup_jacobian()
    assert np.array_equal(rp, d["rp"]) and np.array_equal(ci, d["ci"])
    sim.set_jacobian_values(d["val"])
    assert sim.pc_setup() == 0
    if pc == "bjacobi":
        assert sim.pc_kernel_name().startswith(BRICK_KERNEL[eos]), sim.pc_kernel_name()
    return d, sim


def oracle_sim(oracle, d, eos, pc):
    osim = ol.OracleSim(oracle, d["lm"], KIND[eos])
    if pc == "none":
        oracle.wo_sim_set_pc_none(osim.h, 1)
    return osim


def driver_opts(driver, restart=None):
    o = dict(ksp_type=driver)
    if restart is not None:
        o["gmres_restart"] = restart
    return o


def fresh_uncapped(eos, pc, b, **opts):
    d, sim = pinned_sim(eos, pc, ksp_rtol=1e-8, ksp_atol=1e-50, ksp_max_its=10000, **opts)
    out = solve(sim, b)
    sim.destroy()
    return out


# (driver, restart, the caps, the restatement's keyword arguments)
CAPS = {"bcgs": (None, (1, 2, 3)), "gmres": (30, (1, 2, 3)), "gmres2": (2, (2, 3, 5)), "lgmres": (3, (2, 3, 5)), "bcgsl": (None, (2, 4))}


@pytest.mark.parametrize("eos,pc", SYSTEMS)
@pytest.mark.parametrize("case", list(CAPS))
def test_iteration_cap(oracle, eos, pc, case, monkeypatch):
    """ksp_rtol 1e-30: the solve stops at the cap with -3 and its = k; x is the reference's k-th iterate and rnorm its
    recursive norm at k; and the uncapped solve that follows on the same context is a fresh context's, bit for bit:
    nothing speculative or pending outlives a solve"""
    driver = case.rstrip("2")
    restart, ks = CAPS[case]
    set_form(monkeypatch, "default")
    d, sim = pinned_sim(eos, pc, **driver_opts(driver, restart))
    b = d["b"]
    want = fresh_uncapped(eos, pc, b, **driver_opts(driver, restart))
    assert want[1] == 2, want[:3]
    if driver in ("bcgs", "gmres"):
        kw = dict(merged=True) if driver == "bcgs" else dict(restart=restart)
        dx, dr = se.double_distance(d["M"], d["rb"], driver, ks, **kw)
        assert dx <= 1e-10 and dr <= 1e-10
    else:
        osim = oracle_sim(oracle, d, eos, pc)
    for k in ks:
        sim.set_opts(ksp_rtol=1e-30, ksp_max_its=k)
        its, reason, rn, x = solve(sim, b)
        assert (reason, its) == (-3, k), (case, k, reason, its)
        if driver in ("bcgs", "gmres"):
            ref = (se.bcgs if driver == "bcgs" else se.gmres)(d["M"], d["rb"], rtol=1e-30, maxits=k, **kw)
            ex, er = se.distance(x, ref[3]), abs(rn - float(ref[2])) / float(ref[2])
            print("%s %s %s k=%d: x %.2e (bound %.2e)  rnorm %.2e (bound %.2e)" % (eos, pc, case, k, ex, 10 * dx, er, 10 * dr))
            assert ex <= 10.0 * dx and er <= 10.0 * dr, (case, k, ex, dx, er, dr)
        else:
            oreason, xo, oits, hist = osim.ksp_solve(d["val"], b, ksp_type=OTYPE[driver], restart=restart or 30, rtol=1e-30, maxits=k)
            assert (oreason, oits) == (-3, k)
            ex, er = se.distance(x, xo), abs(rn - hist[-1]) / hist[-1]
            print("%s %s %s k=%d: x %.2e rnorm %.2e against the oracle" % (eos, pc, case, k, ex, er))
            assert ex < OTOL[driver] and er < OTOL[driver], (case, k, ex, er)
        sim.set_opts(ksp_rtol=1e-8, ksp_max_its=10000)
        assert same(solve(sim, b), want), (case, k)
    if driver not in ("bcgs", "gmres"):
        osim.close()
    sim.destroy()


@pytest.mark.parametrize("eos,pc", SYSTEMS)
@pytest.mark.parametrize("form", [f for f in BCGS_FORMS if f != "default"])
def test_iteration_cap_in_every_bicgstab_launch_form(eos, pc, form, monkeypatch):
    """the same for every form a BiCGStab iteration is launched in; WAI_BCGS=petsc reduces (R,R) from R itself, the others
    derive it: each is held to the restatement in its own form"""
    set_form(monkeypatch, form)
    d, sim = pinned_sim(eos, pc, ksp_type="bcgs")
    b = d["b"]
    want = fresh_uncapped(eos, pc, b, ksp_type="bcgs")
    merged = form != "petsc"
    dx, dr = se.double_distance(d["M"], d["rb"], "bcgs", (1, 2, 3), merged=merged)
    for k in (1, 2, 3):
        sim.set_opts(ksp_rtol=1e-30, ksp_max_its=k)
        its, reason, rn, x = solve(sim, b)
        assert (reason, its) == (-3, k), (form, k, reason, its)
        ref = se.bcgs(d["M"], d["rb"], rtol=1e-30, maxits=k, merged=merged)
        ex, er = se.distance(x, ref[3]), abs(rn - float(ref[2])) / float(ref[2])
        print("%s %s %s k=%d: x %.2e (bound %.2e)  rnorm %.2e (bound %.2e)" % (eos, pc, form, k, ex, 10 * dx, er, 10 * dr))
        assert ex <= 10.0 * dx and er <= 10.0 * dr, (form, k, ex, dx, er, dr)
        sim.set_opts(ksp_rtol=1e-8, ksp_max_its=10000)
        assert same(solve(sim, b), want), (form, k)
    sim.destroy()


@pytest.mark.parametrize("eos,pc", SYSTEMS)
@pytest.mark.parametrize("driver", DRIVERS)
def test_tolerance_decides(oracle, eos, pc, driver):
    """ksp_rtol 1e-8 ends with 2; ksp_atol above the reference's first tested residual ends with 3 at the reference's
    iteration; the returned rnorm against the long-double |B^-1 (b - A x)| of the returned x within 10 x the oracle's own
    gap (not less than 2^-53), relative to |B^-1 b|"""
    restart = 3 if driver == "lgmres" else None
    d, sim = pinned_sim(eos, pc, **driver_opts(driver, restart))
    osim = oracle_sim(oracle, d, eos, pc)
    b, M, rb = d["b"], d["M"], d["rb"]
    nb = float(np.sqrt(rb @ rb))
    okw = dict(ksp_type=OTYPE[driver], restart=restart or 30, maxits=10000)
    if driver == "bcgs":
        first = float(se.bcgs(M, rb, rtol=1e-30, maxits=1)[2])
    elif driver == "gmres":
        first = float(se.gmres(M, rb, rtol=1e-30, maxits=1)[2])
    else:
        h = osim.ksp_solve(d["val"], b, rtol=1e-30, **dict(okw, maxits=2))[3]
        first = float(h[2] if driver == "bcgsl" else h[1])
    for tag, rtol, atol, want_reason in (("rtol", 1e-8, 1e-50, 2), ("atol", 1e-30, 1.5 * first, 3)):
        sim.set_opts(ksp_rtol=rtol, ksp_atol=atol, ksp_max_its=10000)
        its, reason, rn, x = solve(sim, b)
        oreason, xo, oits, hist = osim.ksp_solve(d["val"], b, rtol=rtol, atol=atol, **okw)
        assert reason == want_reason == oreason, (driver, tag, reason, oreason)
        if driver in ("bcgs", "gmres"):
            ref = (se.bcgs if driver == "bcgs" else se.gmres)(M, rb, rtol=rtol, atol=atol)[:2]
            assert reason == ref[0] and (its == ref[1] or tag == "rtol"), (tag, its, ref)
        if tag == "atol":
            assert its == oits == (2 if driver == "bcgsl" else 1), (driver, its, oits)
        else:
            assert abs(its - oits) <= max(2, oits // 10), (driver, its, oits)
        true = float(np.sqrt(((rb - M @ x.astype(LD)) ** 2).sum()))
        otrue = float(np.sqrt(((rb - M @ xo.astype(LD)) ** 2).sum()))
        gap, ogap = abs(rn - true) / nb, abs(hist[-1] - otrue) / nb
        print("%s %s %s %s: its %d (oracle %d) rnorm %.6e true %.6e gap %.2e (oracle %.2e)" % (eos, pc, driver, tag, its, oits, rn, true, gap, ogap))
        assert gap <= 10.0 * max(ogap, 2.0 ** -53), (driver, tag, gap, ogap)
    sim.destroy(); osim.close()


@pytest.mark.parametrize("eos,pc", SYSTEMS)
def test_zero_right_hand_side(eos, pc):
    d, sim = pinned_sim(eos, pc)
    for driver in DRIVERS:
        sim.set_opts(**driver_opts(driver, 3 if driver == "lgmres" else None))
        its, reason, rn, x = solve(sim, np.zeros(sim.num_dof))
        assert (reason, its, rn) == (3, 0, 0.0) and not x.any(), (driver, reason, its, rn)
    sim.destroy()


@pytest.mark.parametrize("eos", ["w", "we", "wce", "wsce"])
@pytest.mark.parametrize("pc", ["bjacobi", "none"])
def test_solved_in_one_step(oracle, eos, pc, monkeypatch):
    """A = diag(2^k I) and b = A x with 64 entries of x +-1: under any ILU B^-1 A = I and B^-1 b = x exactly, (x, x) = 64 in
    any order.  BiCGStab: alpha = 1, S = 0, (T,T) = 0 with a zero norm -- 3 at its 1; GMRES and LGMRES: h_00 = 1, h_10 = 0 --
    3 at the first column, v_1 scaled by 1 / 0 and never used.  BiCGStab(2) tests the norm only after a sweep of two BiCG
    steps: the first step solves the system, the second meets (r_1, r~) = 0 and then (u_2, r~) = 0 -- the oracle's
    ksp_type 2 reports a breakdown (-5 at its 0) on this system, and the device must report what the oracle does, with
    x = A^-1 b all the same and no NaN in it.  The preconditioner under pc none is the identity, so there the system is
    A = I.  Then a sound system on the same context, bit for bit a fresh context's"""
    bs = BS[eos]
    lm, rp, ci = se.box(eos)
    xs = se.unit_norm_solution(lm.n_owned, bs)
    val = se.pow2_block_diagonal(rp, ci, bs) if pc == "bjacobi" else np.where(se.pow2_block_diagonal(rp, ci, bs) != 0.0, 1.0, 0.0)
    b = se.dense(rp, ci, val, bs, np.float64) @ xs
    sound = se.diag_dominant_values(rp, ci, bs)
    bsound = np.random.default_rng(7).normal(size=b.size)
    forms = {"bcgs": [f for f in BCGS_FORMS], "gmres": ["default"], "lgmres": ["default"], "bcgsl": ["default"]}
    for driver in DRIVERS:
        opts = dict(pc_type=pc, ksp_rtol=1e-8, **driver_opts(driver, 3 if driver == "lgmres" else None))
        for form in forms[driver]:
            set_form(monkeypatch, form)
            fresh = new_sim(lm, eos, **opts)
            fresh.set_jacobian_values(sound)
            want = solve(fresh, bsound)
            fresh.destroy()
            sim = new_sim(lm, eos, **opts)
            sim.set_jacobian_values(val)
            its, reason, rn, x = solve(sim, b)
            assert not np.isnan(x).any(), (driver, form)
            if driver != "bcgsl":
                assert (reason, its, rn) == (3, 1, 0.0), (driver, form, reason, its, rn)
                assert np.array_equal(x, xs), (driver, form, np.abs(x - xs).max())
            else:
                osim = ol.OracleSim(oracle, lm, KIND[eos])
                if pc == "none":
                    oracle.wo_sim_set_pc_none(osim.h, 1)
                oreason, xo, oits, hist = osim.ksp_solve(val, b, ksp_type=2, rtol=1e-8)
                osim.close()
                print("BiCGStab(2) on the one-step system:", eos, pc, (reason, its, rn), "oracle", (oreason, oits))
                assert (reason, its) == (oreason, oits), (reason, its, oreason, oits)
                assert np.array_equal(x, xs) and np.array_equal(xo, xs)
            sim.set_jacobian_values(sound)
            assert same(solve(sim, bsound), want), (driver, form)
            sim.destroy()


def test_breakdown_on_the_skew_chain(oracle, monkeypatch):
    """bs 1, 64 x 1 x 1, A[i, i+1] = 1, A[i+1, i] = -1, no diagonal, b = ones, pc none: (A r, r) = 1 - 1 + exact zeros.
    BiCGStab: -5 at its 1 in every launch form.  BiCGStab(2): the oracle's ksp_type 2 reports -5 on this system (at its 0:
    the first (u_1, r~) vanishes), and so must the device.  GMRES(30) and LGMRES at a cap of 40: the restatement's and the
    oracle's reason (-3: the residual stagnates) and iteration.  And the next solve is a fresh context's"""
    g, lm, prim, region = make_case(dims=(64, 1, 1), brick=(16, 1, 1), eos="w", lens=False)
    rp, ci = se.mesh_pattern(lm)
    S = se.skew_chain_values(rp, ci)
    ones = np.ones(64)
    sound = se.diag_dominant_values(rp, ci, 1)
    osim = ol.OracleSim(oracle, lm, 0)
    oracle.wo_sim_set_pc_none(osim.h, 1)
    M = se.dense(rp, ci, S, 1)
    for driver, forms in (("bcgs", list(BCGS_FORMS)), ("bcgsl", ["default"]), ("gmres", ["default"]), ("lgmres", ["default"])):
        for form in forms:
            set_form(monkeypatch, form)
            opts = dict(pc_type="none", ksp_max_its=40, **driver_opts(driver, 3 if driver == "lgmres" else None))
            fresh = new_sim(lm, "w", **opts)
            fresh.set_jacobian_values(sound)
            want = solve(fresh, ones)
            fresh.destroy()
            sim = new_sim(lm, "w", **opts)
            rps, cis = sim.setup_jacobian()
            assert np.array_equal(rp, rps) and np.array_equal(ci, cis)
            sim.set_jacobian_values(S)
            its, reason, rn, x = solve(sim, ones)
            oreason, xo, oits, hist = osim.ksp_solve(S, ones, ksp_type=OTYPE[driver], restart=3 if driver == "lgmres" else 30, maxits=40)
            print("skew chain:", driver, form, (reason, its, rn), "oracle", (oreason, oits, hist[-1]))
            if driver == "bcgs":
                assert (reason, its) == (-5, 1) == se.bcgs(M, ones, maxits=40)[:2], (form, reason, its)
                assert oreason == -5
            elif driver == "bcgsl":
                assert oreason == -5 and reason == -5, (reason, its, oreason, oits)
            else:
                if driver == "gmres":
                    ref = se.gmres(M, ones, maxits=40)
                    assert (reason, its) == ref[:2], (reason, its, ref[:2])
                    assert abs(rn - float(ref[2])) <= 1e-12 * float(ref[2])
                assert (reason, its) == (oreason, oits), (driver, reason, its, oreason, oits)
            sim.set_jacobian_values(sound)
            assert same(solve(sim, ones), want), (driver, form)
            sim.destroy()
    osim.close()


@pytest.mark.parametrize("eos,pc", SYSTEMS)
def test_nan_in_the_right_hand_side(eos, pc, monkeypatch):
    """the header's -9: one NaN in b, the matrix sound; every driver (BiCGStab in every launch form) ends with -9, and the
    next clean solve on the context is a fresh context's, bit for bit"""
    d = se.dominant(eos, pc)
    bad = d["b"].copy()
    bad[bad.size // 3] = np.nan
    for driver in DRIVERS:
        for form in (list(BCGS_FORMS) if driver == "bcgs" else ["default"]):
            set_form(monkeypatch, form)
            opts = dict(ksp_rtol=1e-8, **driver_opts(driver, 3 if driver == "lgmres" else None))
            want = fresh_uncapped(eos, pc, d["b"], **driver_opts(driver, 3 if driver == "lgmres" else None))
            d, sim = pinned_sim(eos, pc, **opts)
            its, reason, rn, x = solve(sim, bad)
            assert reason == -9, (driver, form, reason, its, rn)
            assert same(solve(sim, d["b"]), want), (driver, form)
            sim.destroy()


# ---- k. the advisor's open item: last_iteration_fluid after the fused Newton step -------------------------------------------------
def test_last_iteration_fluid_is_refused_after_newton_step_until_pre_iteration():
    from waiwera_amd.lib import LIB, WaiError
    g, lm, prim, region = make_case(dims=(4, 4, 4), brick=(2, 2, 2), eos="we", lens=False)
    sim = new_sim(lm, "we")
    sim.set_regions(region)
    n, dt = sim.num_dof, 1.0e4
    y = scaled(prim, region, "we").ravel().copy()
    assert sim.pre_eval(0.0, y) == 0
    L, f = np.zeros(n), np.zeros(n)
    sim.lhs(0.0, 0.0, y, L)
    assert sim.residual(0.0, dt, y, L, f) == 0
    assert sim.pre_iteration() == 0
    assert np.array_equal(sim.fluid(1), sim.fluid(0))
    reason, kits, mr = sim.newton_step(0.0, dt, 0, y, L, f)
    assert reason >= 0 and kits > 0
    out = np.zeros((sim.n_local, sim.fluid_dof))
    assert LIB.wai_get_fluid(sim.h, 1, out.ctypes.data) == -2
    text = LIB.wai_last_error(sim.h).decode()
    assert "wai_pre_iteration" in text, text
    with pytest.raises(WaiError):
        sim.fluid(1)
    sim.fluid(0)                                   # the state in force is not refused
    assert sim.pre_iteration() == 0
    assert np.array_equal(sim.fluid(1), sim.fluid(0))
    sim.destroy()


# ---- j. two ranks: the pivot fails on rank 1 alone (last: the only case here with more than one process) ------------------------
def _singular_rank_worker(rank, world, uid_q, q):
    from tests import test_hip_multirank as mr
    from waiwera_amd import mesh as M
    os.environ["WAI_RCCL_LIB"] = mr.LOOPBACK
    mr._own_cus(rank, world)
    mr._default_overlap()
    from waiwera_amd import lib as wl
    from waiwera_amd.flow_simulation import FlowSimulation
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=120)
    g, lm, prim, region = mr._problem(M.partition_shape(world), rank, (8, 4, 4), (4, 2, 2))
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.comm_init(rank, world, uid)
    rp, ci = sim.setup_jacobian()
    n = lm.n_owned * 2
    # the pattern's columns reach the ghost cells; diagonal blocks where column == row
    val = se.diag_dominant_values(rp, ci, 2)
    bad = se.singular_at(val, rp, ci, lm.n_owned // 2, 2) if rank == 1 else val
    b = np.random.default_rng(7 + rank).normal(size=n)
    out = []
    sim.set_jacobian_values(bad)
    out.append(("setup", sim.pc_setup()))
    for again in range(2):
        x = np.full(n, 7.0)
        its, reason, rn = sim.ksp_solve(b, x)
        out.append(("solve", reason, its, rn, bool(x.any())))
    z = np.full(n, 3.0)
    out.append(("apply", sim.pc_apply(b, z), bool(np.all(z == 3.0))))
    sim.set_jacobian_values(val)
    out.append(("setup", sim.pc_setup()))
    x = np.zeros(n)
    its, reason, rn = sim.ksp_solve(b, x)
    out.append(("sound", reason, its))
    q.put((rank, out))
    sim.destroy()


@pytest.mark.timeout(300)
def test_two_ranks_singular_pivot_on_one_rank():
    """over the loop-back transport: the pivot fails on rank 1 only, and BOTH ranks return 1 from wai_pc_setup and
    wai_pc_apply and -11 from wai_ksp_solve (fetch_flags all-reduces the flags), twice; then both solve the sound system"""
    import torch.multiprocessing as mp
    from tests import test_hip_multirank as mr
    assert os.path.exists(mr.LOOPBACK), "build first: python __graft_entry__.py"
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_singular_rank_worker, args=(r, 2, uid_q, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=200) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for p in procs:
        assert p.exitcode == 0
    for rank in (0, 1):
        out = res[rank]
        assert out[0] == ("setup", 1), (rank, out)
        assert out[1] == out[2] == ("solve", -11, 0, 0.0, False), (rank, out)
        assert out[3] == ("apply", 1, True), (rank, out)
        assert out[4] == ("setup", 0) and out[5][1] > 0, (rank, out)
    assert res[0][5][1:] == res[1][5][1:]
