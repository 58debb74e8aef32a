"""PCASM (restricted, any overlap, sub-preconditioner ILU(k), k >= 0) applied in one fused launch: k_pc_wide's two-pattern
form with a row map -- A x on the Jacobian's planes at the operator's row ext_row[q], the two sweeps on the extended
system's own planes at the factor's row q, the rows a block owns written back and reduced -- wherever every extended block
has at most 1024 rows and every row of E at most 16 blocks (meshes of at most 8 blocks per row, one rank).

The shapes (tests/asm_reference.py, CASES) are the smallest at which the kernel can go wrong; each one's largest extended
block and widest row are computed on the CPU (tests/test_asm_reference.py asserts them without a GPU, the tests here
assert them again on the pattern the library reports).

Bars.  One application at a time against the long-double reference of tests/asm_reference.py with the bars of
tests/test_hip_fused_operator.py's Checker: z within 1e-12 of max|z_ref|, an inner product within 1e-13 of sum |a_i b_i|,
three identical applications bit-identical, slots a phase does not write untouched.  Fused against today's launches on the
same matrix (WAI_ASM_UNFUSED=1: k_spmv, gather, k_pc on the extended system in DILU form, scatter): 1e-10 of max|z|, the
bar tests/test_hip_iluk_fused.py holds the same comparison to.  Whole solves against the oracle's PCASM on the same
subdomains: the same reason, iteration counts within one, solutions within 1e-7.

The fallback build (tools/ci_fallback_kernels.sh) replaces the narrow brick kernels only: wide schedules keep k_pc_wide
there, so the names expected here are the same in both builds."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as ol
from tests import asm_reference as ar
from tests import fused_reference as fr
from tests import test_hip_fused_operator as fo
from waiwera_amd.cases import make_case, scaled
from waiwera_amd.lib import WaiError

pytestmark = pytest.mark.gpu

KIND, BS = fo.KIND, fo.BS
CASES, TOO_BIG = ar.CASES, ar.TOO_BIG
UNFUSED = "k_spmv + "


def fused_name(bs, levels):
    return "k_pc_wide<%d,spmv,map> on the extended system (ASM, ILU(%d))" % (bs, levels)


def relmax(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


_systems = {}


def system(oracle, key):
    """mesh, FD Jacobian of the case's state, right-hand side and the reference's pattern: computed once per shape and shared
    (nothing here is modified by a test)"""
    eos, dims, brick, overlap, levels = key
    if key not in _systems:
        g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=(eos == "we"))
        rp, ci, J = fo.fd_jacobian(oracle, lm, eos, prim, region)
        osim = ol.OracleSim(oracle, lm, KIND[eos])
        osim.set_regions(region)
        yo = osim.yvec(scaled(prim, region, eos).ravel().copy())
        assert osim.pre_eval(yo) == 0
        err, f = osim.residual(yo, 5.0e4, osim.lhs())
        osim.close()
        pat = ar.AsmPattern(rp, ci, np.asarray(lm.sub_ptr), overlap, levels)
        _systems[key] = dict(lm=lm, prim=prim, region=region, rp=rp, ci=ci, J=J, f=f, pat=pat)
    return _systems[key]


def make_sim(S, key, **opts):
    from waiwera_amd.flow_simulation import FlowSimulation
    eos, dims, brick, overlap, levels = key
    sim = FlowSimulation(S["lm"], eos=eos)
    sim.set_regions(S["region"])
    sim.set_opts(pc_type="asm", asm_overlap=overlap, ilu_levels=levels, **opts)
    sim.set_jacobian_values(S["J"])
    return sim


class AsmChecker(fo.Checker):
    def __init__(self, sim, pat, bs, val, label):
        self.sim, self.bs, self.val, self.label = sim, bs, val, label
        sim.set_jacobian_values(val)
        assert sim.pc_setup() == 0
        self.ref = ar.AsmRef(pat, val, bs)
        rng = np.random.default_rng(11)
        self.x, self.x2, self.aux = (fr.spread_vector(pat.n, bs, rng) for _ in range(3))
        s = np.zeros(16)
        s[fr.S_RHO], s[fr.S_RHOOLD], s[fr.S_OMEGA], s[fr.S_BETA] = 0.83, 1.7, 0.61, 2.3
        s[fr.S_D1:fr.S_W2 + 1] = rng.normal(size=5)   # stale sums: whatever a mode does not write must survive
        s[10:15] = rng.normal(size=5)
        s[fr.S_ALPHA] = fo.ALPHA
        self.scal_in = s
        self.rows = {}


@pytest.mark.parametrize("case", list(CASES))
def test_routing(oracle, case, monkeypatch):
    """pc_kernel_name() names the mapped form for every fused case and today's launches under WAI_ASM_UNFUSED=1; block Jacobi
    on the same context keeps the kernel it had, and PCASM comes back fused"""
    key = CASES[case]
    eos, levels = key[0], key[4]
    S = system(oracle, key)
    assert S["pat"].max_rows <= 1024 and S["pat"].width <= 16
    sim = make_sim(S, key)
    sim.set_opts(pc_type="bjacobi", ilu_levels=0)
    assert sim.pc_setup() == 0
    brick_kernel = sim.pc_kernel_name()
    assert "extended" not in brick_kernel and "map" not in brick_kernel, brick_kernel
    sim.set_opts(pc_type="asm", ilu_levels=levels)
    assert sim.pc_setup() == 0
    name = sim.pc_kernel_name()
    assert name == fused_name(BS[eos], levels), name
    assert not sim.pc_axpy_capable()          # no composed operand: BiCGStab takes the four-launch form
    monkeypatch.setenv("WAI_ASM_UNFUSED", "1")
    assert sim.pc_setup() == 0
    name = sim.pc_kernel_name()
    assert name.startswith(UNFUSED) and "on the extended system (ASM, ILU(%d))" % levels in name and "map" not in name, name
    assert not sim.pc_axpy_capable()
    monkeypatch.delenv("WAI_ASM_UNFUSED")
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(BS[eos], levels)
    sim.set_opts(pc_type="bjacobi", ilu_levels=0)
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == brick_kernel, sim.pc_kernel_name()
    sim.set_opts(pc_type="asm", ilu_levels=levels)
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(BS[eos], levels)
    # the probes of one kernel class assume a factor on the system's own rows: refused, not run out of bounds
    for which in (9, 10, 16, 23):
        with pytest.raises(WaiError):
            sim.bench_kernel(which, reps=1)
    sim.destroy()


def test_routing_keeps_todays_launches_for_the_bench_brick():
    """an interior 16 x 16 x 2 brick extends to 1152 rows: more than one workgroup, so today's path, by its old name"""
    from waiwera_amd.flow_simulation import FlowSimulation
    eos, dims, brick, overlap, levels = TOO_BIG
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=True)
    sim = FlowSimulation(lm, eos=eos)
    sim.set_regions(region)
    sim.set_opts(pc_type="asm", asm_overlap=overlap, ilu_levels=levels)
    rp, ci = sim.setup_jacobian()
    pat_rows = np.diff(ar.extended_sets(rp, ci, np.asarray(lm.sub_ptr), overlap)[0]).max()
    assert pat_rows == 1152
    y = scaled(prim, region, eos).ravel().copy()
    L = np.zeros(sim.num_dof)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, 1.0, y, L)
    assert sim.jacobian(0.0, 5.0e4, y, L) == 0
    assert sim.pc_setup() == 0
    name = sim.pc_kernel_name()
    assert name.startswith(UNFUSED) and "on the extended system (ASM, ILU(0))" in name and "map" not in name, name
    sim.destroy()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", list(CASES))
def test_one_application_against_long_double_reference(oracle, case):
    """z = B^-1 A x and z = B^-1 x, dot modes 0 - 4, the reductions finished in the launch and by k_finalize, on the FD
    Jacobian and on random O(1) values; what the kernel cannot serve (a composed operand, the interior / face split) is
    refused, not answered.  Every case meets Checker's own bars (z 1e-12, products 1e-13)."""
    key = CASES[case]
    eos, levels = key[0], key[4]
    bs = BS[eos]
    S = system(oracle, key)
    rp, ci, pat = S["rp"], S["ci"], S["pat"]
    assert pat.max_rows <= 1024 and pat.width <= 16
    sim = make_sim(S, key)
    rps, cis = sim.setup_jacobian()
    assert np.array_equal(rp, rps) and np.array_equal(ci, cis)
    for values in ("fd", "random"):
        val = S["J"] if values == "fd" else fr.random_values(rp, ci, bs, np.random.default_rng(12))
        ck = AsmChecker(sim, pat, bs, val, (case, values))
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
        ck.report(kernel)
    sim.destroy()


class DeviceVectors:
    """device copies of host vectors, through the HIP runtime the library itself links (blocking copies)"""

    def __init__(self, *hosts):
        self.hosts, self.ptrs = [np.ascontiguousarray(h, dtype=np.float64) for h in hosts], []

    @staticmethod
    def _hip():
        from waiwera_amd.lib import LIB
        LIB.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        LIB.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        LIB.hipFree.argtypes = [C.c_void_p]
        return LIB

    def __enter__(self):
        hip = self._hip()
        for h in self.hosts:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), h.nbytes) == 0
            self.ptrs.append(p)
            assert hip.hipMemcpy(p, h.ctypes.data, h.nbytes, 1) == 0    # hipMemcpyHostToDevice
        return self.ptrs

    def __exit__(self, *exc):
        for p in self.ptrs:
            self._hip().hipFree(p)

    @classmethod
    def fetch(cls, p, n):
        out = np.empty(n)
        assert cls._hip().hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0     # hipMemcpyDeviceToHost
        return out


@pytest.mark.parametrize("case", ["we_ragged", "wce_ragged", "we_overlap2"])
def test_locality_and_restriction(oracle, case):
    """x non-zero in one brick only: every owned row of a block whose extended set holds no non-zero entry of t (t = x, or
    t = A x) comes back exactly 0.0.  And one application into a z pre-filled with NaN leaves every entry finite: each row
    is written by the block that owns it, nothing is left out; applied in place it is refused"""
    key = CASES[case]
    eos = key[0]
    bs = BS[eos]
    S = system(oracle, key)
    rp, ci, pat = S["rp"], S["ci"], S["pat"]
    sub = np.asarray(S["lm"].sub_ptr)
    n, nb = pat.n, len(sub) - 1
    sim = make_sim(S, key)
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(bs, key[4])
    ref = ar.AsmRef(pat, S["J"], bs)
    x = fr.spread_vector(n, bs, np.random.default_rng(21))
    b = 0                                # a corner brick: the far corner's blocks cannot be reached
    xl = np.zeros(n * bs)
    xl[sub[b] * bs:sub[b + 1] * bs] = x[sub[b] * bs:sub[b + 1] * bs]
    rows = np.repeat(np.arange(n), np.diff(rp))
    for spmv in (False, True):
        live = np.zeros(n, dtype=bool)       # rows where t can be non-zero
        if spmv:
            live[np.unique(rows[(ci >= sub[b]) & (ci < sub[b + 1])])] = True
        else:
            live[sub[b]:sub[b + 1]] = True
        quiet = [s for s in range(nb) if not live[pat.ext_row[pat.ext_ptr[s]:pat.ext_ptr[s + 1]]].any()]
        assert quiet, case
        z, _ = sim.pc_operator(xl, spmv=spmv)
        for s in quiet:
            assert np.all(z[sub[s] * bs:sub[s + 1] * bs] == 0.0), (case, spmv, s)
        zref = ref.operator(S["J"], xl) if spmv else ref.solve(xl)
        assert fo.relerr(z, zref) <= 1e-12
    with DeviceVectors(x, np.full(x.size, np.nan)) as (r, z):
        sim.pc_apply(r.value, z.value)       # device pointers: applied where they are, z as it stands
        sim.synchronize()
        zh = DeviceVectors.fetch(z, x.size)
        with pytest.raises(WaiError):
            sim.pc_apply(r.value, r.value)
    assert np.isfinite(zh).all()
    assert fo.relerr(zh, ref.solve(x)) <= 1e-12
    sim.destroy()


@pytest.mark.parametrize("case", list(CASES))
def test_against_todays_launches(oracle, case, monkeypatch):
    """the same matrix factored and applied by the launches this replaces (WAI_ASM_UNFUSED=1): applications within 1e-10;
    the fused form applied again afterwards gives the bits it gave first"""
    key = CASES[case]
    eos = key[0]
    S = system(oracle, key)
    n = S["pat"].n
    sim = make_sim(S, key)
    rng = np.random.default_rng(5)
    r, x = rng.normal(size=n * BS[eos]), fr.spread_vector(n, BS[eos], rng)
    out = {}
    for path in ("fused", "unfused", "again"):
        if path == "unfused":
            monkeypatch.setenv("WAI_ASM_UNFUSED", "1")
        if path == "again":
            monkeypatch.delenv("WAI_ASM_UNFUSED")
        assert sim.pc_setup() == 0
        name = sim.pc_kernel_name()
        assert ("map" in name) == (path != "unfused") and name.startswith(UNFUSED) == (path == "unfused"), (path, name)
        z = np.zeros(n * BS[eos])
        sim.pc_apply(r, z)
        out[path] = (z, sim.pc_operator(x, spmv=True)[0])
    for a, b in zip(out["fused"], out["unfused"]):
        print(case, "fused against unfused", relmax(a, b))
        assert relmax(a, b) < 1e-10
    for a, b in zip(out["fused"], out["again"]):
        assert np.array_equal(a, b)
    sim.destroy()


@pytest.mark.parametrize("case", ["we_ragged", "wce_ragged"])
@pytest.mark.parametrize("ksp,kt", [("bcgs", 0), ("gmres", 1)])
def test_whole_solves_against_the_oracle(oracle, case, ksp, kt):
    """BiCGStab and GMRES under fused PCASM at rtol 1e-10 against the oracle's solves with PCASM, overlap 1, on the same
    subdomains"""
    key = CASES[case]
    eos = key[0]
    S = system(oracle, key)
    n = S["pat"].n
    sim = make_sim(S, key, ksp_type=ksp, ksp_rtol=1e-10)
    osim = ol.OracleSim(oracle, S["lm"], KIND[eos])
    osim.set_regions(S["region"])
    osim.set_asm(1)
    assert sim.pc_setup() == 0 and osim.pc_setup(S["J"]) == 0
    assert sim.pc_kernel_name() == fused_name(BS[eos], 0)
    x = np.zeros(n * BS[eos])
    its, reason, rn = sim.ksp_solve(S["f"], x)
    oreason, xo, oits, hist = osim.ksp_solve(S["J"], S["f"], ksp_type=kt, rtol=1e-10)
    print(case, ksp, "its", its, oits, "reason", reason, oreason, "x", relmax(x, xo[:x.size]))
    assert reason > 0 and reason == oreason, (reason, oreason)
    assert abs(its - oits) <= 1, (its, oits)
    assert relmax(x, xo[:x.size]) < 1e-7
    sim.destroy(); osim.close()


def test_bicgstab_iteration_is_four_launches(oracle, monkeypatch):
    """one BiCGStab iteration under fused PCASM: fused A P, S = R - alpha V, fused A S, the X / R / P update -- four launches
    by the library's counter (+ the solve's set-up and the speculative half iteration that is thrown away).  The same solve
    by today's launches is printed beside it"""
    key = CASES["we_ragged"]
    S = system(oracle, key)
    n = S["pat"].n
    sim = make_sim(S, key, ksp_type="bcgs", ksp_rtol=1e-10)
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(2, 0)
    x = np.zeros(n * 2)
    k0, c0 = sim.launch_stats()
    its, reason, rn = sim.ksp_solve(S["f"], x)
    k1, c1 = sim.launch_stats()
    monkeypatch.setenv("WAI_ASM_UNFUSED", "1")
    assert sim.pc_setup() == 0
    xu = np.zeros(n * 2)
    u0, _ = sim.launch_stats()
    uits, ureason, _ = sim.ksp_solve(S["f"], xu)
    u1, _ = sim.launch_stats()
    print("BiCGStab on we_ragged: fused %d launches in %d iterations, unfused %d launches in %d iterations"
          % (k1 - k0, its, u1 - u0, uits))
    assert reason > 0 and its >= 5
    assert 4 * its <= k1 - k0 <= 4 * its + 8, (its, k1 - k0)
    sim.destroy()


def test_timestep_against_todays_launches(monkeypatch):
    """one backward-Euler step under PCASM on 8 x 8 x 6 in 4 x 4 x 2 bricks, fused against WAI_ASM_UNFUSED=1, both at
    ksp_rtol 1e-12: the Newton iterates then do not depend on how the preconditioner is applied -- same Newton count,
    solution within 1e-9 relative"""
    from waiwera_amd.flow_simulation import FlowSimulation
    res = {}
    for tag in ("fused", "unfused"):
        if tag == "unfused":
            monkeypatch.setenv("WAI_ASM_UNFUSED", "1")
        g, lm, prim, region = make_case(dims=(8, 8, 6), brick=(4, 4, 2), eos="we", lens=True)
        sim = FlowSimulation(lm, eos="we")
        sim.set_regions(region)
        sim.set_opts(pc_type="asm", asm_overlap=1, ilu_levels=0, ksp_rtol=1e-12, ftol_rel=1e-9)
        y = scaled(prim, region, "we").ravel().copy()
        reason, nits, kits = sim.timestep(0.0, 1.0e4, y)
        name = sim.pc_kernel_name()
        assert reason > 0 and ("map" in name) == (tag == "fused") and "ASM" in name, (tag, reason, name)
        res[tag] = (nits, y.reshape(-1, 2).copy(), kits)
        sim.destroy()
    print("timestep: Newton", res["fused"][0], res["unfused"][0], "Krylov", res["fused"][2], res["unfused"][2])
    assert res["fused"][0] == res["unfused"][0]
    yf, yu = res["fused"][1], res["unfused"][1]
    err = np.abs(yf - yu).max(axis=0) / np.abs(yu).max(axis=0)
    print("timestep: fused against unfused", err)
    assert err.max() < 1e-9, err
