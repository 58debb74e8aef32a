"""Each fused preconditioned-operator launch against the long-double reference of tests/fused_reference.py, one application
at a time (wai_test_pc_operator: the application exactly as the Krylov drivers issue it).

Every kernel kind and template variant pc_kernel_kind / build_schedule can select is reached by one case of CASES, at the
brick shapes where the kernels change behaviour; each case runs on the oracle's FD Jacobian of the case's state and on
random O(1) values on the same pattern (blocks that are structurally zero in single-phase cells filled too).  Per case:
z = B^-1 A (x - alpha x2) and z = B^-1 x, dot modes 0-4, the composed operand where the kernel can form it, the interior /
face split where the mesh has both lists, the reductions finished by k_finalize (-2), in the launch (-1) and with the
drivers' phases (2 with mode 1, 3 with mode 2, 0 with mode 3, 6 with mode 4).

Bars: z within 1e-12 max|z_ref|; an inner product within 1e-13 sum |a_i b_i|; a derived scalar within 1e-12 of the
restated formula applied to the launch's own sums (relative to the sum of the magnitudes of the formula's terms); every
slot a phase does not write bit-identical to what went in; three identical applications bit-identical.

The *_sliced_* cases (SLICED) leave more than 1024 and more than 2048 partial sums per slot: their reductions are finished
in two and three slices (k_finalize's slice loop, the finaliser workgroups' second-level sums, a short last slice), on the
random-values matrix alone, with the count asserted (wai_test_partial_count).  MEASURED: the same margins as the unsliced
cases (inner products <= 3.2e-16 sum |a_i b_i|, z <= 4.3e-16 max|z_ref|).

tools/ci_fallback_kernels.sh exports WAI_FALLBACK_BUILD=1: that library routes every case through the generic stored-factor
k_pc (no composed operand), and the same comparisons must hold."""
import os

import numpy as np
import pytest

from oracle import binding as ol
from tests import fused_reference as fr
from waiwera_amd.cases import make_case, scaled
from waiwera_amd.lib import WaiError

pytestmark = pytest.mark.gpu

KIND = {"w": 0, "we": 1, "wce": 2, "wsce": 5}
BS = {"w": 1, "we": 2, "wce": 3, "wsce": 4}
FALLBACK = os.environ.get("WAI_FALLBACK_BUILD") == "1"
ALPHA = 0.37
LEVELS = "k_spmv + k_lvl_solve per level"

# id: (eos, dims, brick, make_case extras, kernel name of the default build, environment at the context's creation)
CASES = {
    # 1 x 1 blocks on the generic kernel; bricks ragged in y (10 = 4 + 4 + 2) and z (9 = 4 + 4 + 1)
    "generic_bs1": ("w", (12, 10, 9), (4, 4, 4), {}, "k_pc<1,spmv,dilu-scaled,compact3>", {}),
    # ragged bricks, 45 of them (not a multiple of 8)
    "park_ragged": ("we", (12, 10, 9), (4, 4, 2), {}, "k_pc_park<spmv,col16>", {}),
    # the bench's brick: 512-row bricks (T = 512, k_pc_park's limit) beside ragged 8-wide ones; uneven costs: LPT order
    "park_bench_brick": ("we", (40, 36, 6), (16, 16, 2), {}, "k_pc_park<spmv,col16>", {}),
    # the same on the int32 column planes because the 16-bit indices bail out (a brick reaches too many segments)
    "park_int32_bailout": ("we", (40, 36, 6), (16, 16, 2), {}, "k_pc_park<spmv>", {"WAI_COL16_MAX_SEG": "1"}),
    # 1024-row bricks: past k_pc_park's limit, the generic kernel
    "generic_bs2_1024": ("we", (16, 16, 8), (16, 16, 4), {}, "k_pc<2,spmv,dilu-scaled,compact3>", {}),
    # 1280-row bricks: more than a workgroup, the launch-per-level path (k_lvl_factor / k_lvl_solve, unfused pc_amul).
    # Its FD-Jacobian z error is the largest of the file (3.3e-13 of max|z_ref|, within the 1e-12 bar; random values on
    # the same pattern and kernels: 6e-16): 1280-row triangular sweeps over the lens' two-phase blocks
    "levels_1280": ("we", (16, 16, 10), (16, 16, 5), {}, LEVELS, {}),
    # one wave per brick at the wave limit (64 rows: bench C4's brick)
    "wave_64": ("wce", (24, 12, 4), (8, 4, 2), {}, "k_pc_wave<3,spmv>", {}),
    # ragged in x, y, z; 27 bricks: the last workgroup of four holds 3; padded rows (rp path); one interior brick: split,
    # the face launch's partial-sum indices continue the interior's (pbase)
    "wave_ragged": ("wce", (13, 9, 5), (5, 4, 2), {}, "k_pc_wave<3,spmv>", {}),
    # MINC: long rows, then short ones (sub_split)
    "wave_minc": ("wce", (16, 8, 4), (4, 4, 1), {"minc": True}, "k_pc_wave<3,spmv>", {}),
    # 128-row bricks: past the wave limit
    "rows_3": ("wce", (16, 8, 8), (8, 4, 4), {}, "k_pc_rows<3,spmv,3+3>", {}),
    # MINC bricks of 4 x 4 x 4 cells: an inner fracture cell has x+, y+, z+ and its matrix cell as upper couplings
    # in the brick (max_nlu = 4), 128 rows: past the wave limit
    "rows_3_nlu4": ("wce", (8, 8, 4), (4, 4, 4), {"minc": True}, "k_pc_rows<3,spmv,4+4>", {}),
    # 4 x 4 blocks: 16-row bricks, and 64-row bricks = 256 threads
    "rows_4": ("wsce", (8, 8, 4), (4, 2, 2), {}, "k_pc_rows<4,spmv,3+3>", {}),
    "rows_4_256": ("wsce", (8, 8, 4), (4, 4, 4), {}, "k_pc_rows<4,spmv,3+3>", {}),
    # a cell graph with triangles: off-diagonal fill, the stored factor (DI = 0)
    "stored_factor": ("we", None, None, {}, "k_pc<2,spmv,ilu,compact3>", {}),
    # More than 1024 partial sums per slot: the finalisation in slices (fin_slices; SLICED below).  Two slices, and three with
    # a short last one (2560 = 854 + 854 + 852; 2050 = 684 + 684 + 682), on the generic kernel, k_pc_park and k_pc_wave -- whose
    # partial sums are per workgroup of four bricks: four times the bricks.  Small bricks keep the meshes small
    "generic_sliced_2": ("w", (24, 24, 8), (2, 2, 1), {}, "k_pc<1,spmv,dilu-scaled,compact3>", {}),
    "generic_sliced_3": ("w", (32, 32, 10), (2, 2, 1), {}, "k_pc<1,spmv,dilu-scaled,compact3>", {}),
    "park_sliced_2": ("we", (24, 24, 8), (2, 2, 1), {}, "k_pc_park<spmv,col16>", {}),
    "park_sliced_3": ("we", (32, 32, 10), (2, 2, 1), {}, "k_pc_park<spmv,col16>", {}),
    "wave_sliced_2": ("wce", (34, 32, 16), (2, 2, 1), {}, "k_pc_wave<3,spmv>", {}),
    "wave_sliced_3": ("wce", (20, 20, 41), (2, 1, 1), {}, "k_pc_wave<3,spmv>", {}),
}

# case: (partial sums per reduction slot a launch over all bricks leaves, slices they are finished in).  These cases run on
# the random-values matrix alone: the oracle's FD Jacobian of their meshes would take longer than everything else they do
SLICED = {"generic_sliced_2": (1152, 2), "generic_sliced_3": (2560, 3), "park_sliced_2": (1152, 2), "park_sliced_3": (2560, 3),
          "wave_sliced_2": (1088, 2), "wave_sliced_3": (2050, 3)}


def fin_slices(nb):
    """reductions.hip.h: slices of about 1024 partial sums, at most 64"""
    return 1 if nb <= 1024 else min(64, -(-nb // 1024))

# the drivers' in-launch phases per dot mode (krylov.hip: bcgs_first_half 2, the petsc form's omega 3, do_bcgs's start 0,
# bcgs_second_half 6)
DRIVER_PHASE = {1: 2, 2: 3, 3: 0, 4: 6}


def expected_name(case):
    eos, name = CASES[case][0], CASES[case][4]
    if not FALLBACK or name == LEVELS:
        return name
    return "k_pc<%d,spmv,ilu," % BS[eos]   # (prefix: compact3 or generic depends on the brick's slot layout)


def build(case, monkeypatch):
    from waiwera_amd.flow_simulation import FlowSimulation
    eos, dims, brick, extra, _, env = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if dims is None:
        g, lm, prim, region = fr.triangle_mesh(eos)
    else:
        g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=(eos == "we"), **extra)
    sim = FlowSimulation(lm, eos=eos)
    for k in env:
        monkeypatch.delenv(k)
    return lm, sim, prim, region


def fd_jacobian(oracle, lm, eos, prim, region, dt=5.0e4):
    osim = ol.OracleSim(oracle, lm, KIND[eos])
    osim.set_regions(region)
    yo = osim.yvec(scaled(prim, region, eos).ravel().copy())
    assert osim.pre_eval(yo) == 0
    L = osim.lhs()
    err, f = osim.residual(yo, dt, L)
    err, J = osim.jacobian(yo, dt, L, f, mode=0)
    assert err == 0
    rp, ci = osim.pattern()
    osim.close()
    return rp, ci, J


def relerr(z, zref):
    zr = zref.astype(np.float64)
    return float(np.abs(z - zr).max() / max(np.abs(zr).max(), 1e-300))


class Checker:
    """one matrix on one context: every application compared with the reference, the worst errors kept per variant"""

    def __init__(self, sim, rp, ci, sub, bs, val, label):
        self.sim, self.bs, self.val, self.label = sim, bs, val, label
        sim.set_jacobian_values(val)
        assert sim.pc_setup() == 0
        self.ref = fr.BlockILU0(rp, ci, val, bs, sub)
        n = len(rp) - 1
        rng = np.random.default_rng(11)
        self.x, self.x2, self.aux = (fr.spread_vector(n, bs, rng) for _ in range(3))
        s = np.zeros(16)
        s[fr.S_RHO], s[fr.S_RHOOLD], s[fr.S_OMEGA], s[fr.S_BETA] = 0.83, 1.7, 0.61, 2.3
        s[fr.S_D1:fr.S_W2 + 1] = rng.normal(size=5)   # stale sums: whatever a mode does not write must survive
        s[10:15] = rng.normal(size=5)
        s[fr.S_ALPHA] = ALPHA
        self.scal_in = s
        self.rows = {}

    def apply(self, **kw):
        return self.sim.pc_operator(self.x if "x" not in kw else kw.pop("x"), alpha=ALPHA, scal_in=self.scal_in, **kw)

    def variant(self, tag, spmv, composed, split):
        """all dot modes and finalisations of one form of the application"""
        x2 = self.x2 if composed else None
        if spmv:
            opnd = self.x.astype(fr.LD) - fr.LD(ALPHA) * self.x2.astype(fr.LD) if composed else self.x.astype(fr.LD)
            zref = self.ref.operator(self.val, opnd)
        else:
            opnd = self.x.astype(fr.LD)
            zref = self.ref.solve(self.x)
        worst_z, worst_d, worst_s = 0.0, 0.0, 0.0
        z0 = None
        for mode in range(5):
            kw = dict(x2=x2, dot_mode=mode, aux=self.aux if mode in (1, 4) else None, spmv=spmv, split=split)
            phases = [-2] if mode == 0 else [-2, -1, DRIVER_PHASE[mode]]
            sums = None
            for phase in phases:
                z, s = self.apply(fin_phase=phase, **kw)
                e = relerr(z, zref)
                worst_z = max(worst_z, e)
                assert e <= 1e-12, (self.label, tag, mode, phase, e)
                if z0 is None:
                    z0 = z
                # z does not depend on what is reduced, nor on where: the same launch arithmetic every time
                assert np.array_equal(z, z0), (self.label, tag, mode, phase)
                prods = fr.mode_products(mode, opnd, zref, self.aux)
                written = {slot for slot, _, _ in prods}
                if phase < 0:
                    for slot, a, b in prods:
                        d, bar = fr.dot(a, b)
                        err = abs(s[slot] - float(d)) / float(bar)
                        worst_d = max(worst_d, err)
                        assert err <= 1e-13, (self.label, tag, mode, phase, slot, s[slot], float(d), err)
                    others = [i for i in range(16) if i not in written]
                    assert np.array_equal(s[others], self.scal_in[others]), (self.label, tag, mode, phase, s, self.scal_in)
                    if sums is None:
                        sums = s
                    else:   # k_finalize and the in-launch finalisers add the same partials in the same order: same bits
                        assert np.array_equal(s, sums), (self.label, tag, mode, s - sums)
                else:
                    want, scale = fr.derive(sums, phase)
                    for i in range(16):
                        if i in scale:
                            err = abs(s[i] - want[i]) / max(scale[i], 1e-300)
                            worst_s = max(worst_s, err)
                            assert err <= 1e-12, (self.label, tag, mode, phase, i, s[i], want[i])
                        else:
                            assert s[i] == want[i] or (np.isnan(s[i]) and np.isnan(want[i])), (self.label, tag, mode, phase, i, s[i], want[i])
            if mode == 4:   # repeatability: the in-launch finalisation does not depend on the order partials arrive in
                ph = DRIVER_PHASE[4]
                runs = [self.apply(fin_phase=ph, **kw) for _ in range(3)]
                for z, s in runs[1:]:
                    assert np.array_equal(z, runs[0][0]) and np.array_equal(s, runs[0][1]), (self.label, tag)
        self.rows[tag] = (worst_z, worst_d, worst_s)
        return z0

    def local_input(self, sub, rp, ci):
        """x zero outside one brick: every row outside the bricks the operator can reach comes back exactly 0.0"""
        n = len(rp) - 1
        b = (len(sub) - 1) // 2
        lo, hi = sub[b], sub[b + 1]
        xl = np.zeros(n * self.bs)
        xl[lo * self.bs:hi * self.bs] = self.x[lo * self.bs:hi * self.bs]
        owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
        rows = np.repeat(np.arange(n), np.diff(rp))
        touched = np.unique(rows[(ci >= lo) & (ci < hi)])      # rows of A x that can be nonzero
        for spmv, reach in ((False, {b}), (True, set(owner[touched].tolist()))):
            z, _ = self.sim.pc_operator(xl, spmv=spmv, scal_in=self.scal_in)
            out = ~np.isin(np.repeat(owner, self.bs), list(reach))
            # (on a mesh of two bricks the operator reaches both: nothing left to be zero)
            assert out.any() or spmv, self.label
            assert np.all(z[out] == 0.0), (self.label, spmv, np.abs(z[out]).max() if out.any() else None)
            zref = self.ref.operator(self.val, xl) if spmv else self.ref.solve(xl)
            e = relerr(z, zref)
            assert e <= 1e-12, (self.label, "local", spmv, e)

    def report(self, kernel):
        print()
        for tag, (ez, ed, es) in self.rows.items():
            print("%-22s %-32s %-7s %-16s z %.2e  dots %.2e  scalars %.2e" % (self.label[0], kernel, self.label[1], tag, ez, ed, es))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", list(CASES))
def test_fused_operator_against_long_double_reference(oracle, case, monkeypatch):
    eos = CASES[case][0]
    bs = BS[eos]
    lm, sim, prim, region = build(case, monkeypatch)
    monkeypatch.delenv("WAI_NO_COL16", raising=False)
    kernel = sim.pc_kernel_name()
    want = expected_name(case)
    assert kernel.startswith(want) if FALLBACK else kernel == want, (case, kernel, want)
    if case in SLICED:
        rp, ci = sim.setup_jacobian()
        Jfd = None
    else:
        rp, ci, Jfd = fd_jacobian(oracle, lm, eos, prim, region)
        rps, cis = sim.setup_jacobian()
        assert np.array_equal(rp, rps) and np.array_equal(ci, cis)
    sub = np.asarray(lm.sub_ptr)
    n = len(rp) - 1
    # what this context can serve: the composed operand (k_pc_park / k_pc_rows / k_pc_wave), the interior / face split
    # (fused kernels, one rank, rows of seven blocks, both lists non-empty)
    fused_kind = kernel.startswith(("k_pc_park", "k_pc_rows", "k_pc_wave"))
    assert sim.pc_axpy_capable() == fused_kind
    width = np.diff(rp)
    owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
    face = np.zeros(len(sub) - 1, dtype=bool)
    np.logical_or.at(face, owner, width < 7)
    can_split = kernel != LEVELS and width.max() == 7 and face.any() and not face.all()
    variants = [("B^-1 x", False, False, False), ("B^-1 A x", True, False, False)]
    if fused_kind:
        variants.append(("B^-1 A (x - a x2)", True, True, False))
    if can_split:
        variants.append(("split", True, False, True))
        if fused_kind:
            variants.append(("split composed", True, True, True))
    for values in (("random",) if case in SLICED else ("fd", "random")):
        val = Jfd if values == "fd" else fr.random_values(rp, ci, bs, np.random.default_rng(12))
        ck = Checker(sim, rp, ci, sub, bs, val, (case, values))
        # what the kernel cannot serve is refused, not answered
        if not fused_kind:
            with pytest.raises(WaiError):
                ck.apply(x2=ck.x2)
        with pytest.raises(WaiError):
            ck.apply(x2=ck.x2, spmv=False)
        if not can_split:
            with pytest.raises(WaiError):
                ck.apply(split=True)
        zs = {}
        for tag, spmv, composed, split in variants:
            zs[tag] = ck.variant(tag, spmv, composed, split)
        if fused_kind:
            # x2 = 0: the composed launch forms x - alpha * 0 = x exactly, so its result is the plain launch's, bit for bit
            z0, _ = ck.apply(x2=np.zeros(n * bs))
            assert np.array_equal(z0, zs["B^-1 A x"]), (case, values, relerr(z0, zs["B^-1 A x"].astype(fr.LD)))
        if case == "park_bench_brick":
            # the same context on the int32 column planes (WAI_NO_COL16, read per application)
            monkeypatch.setenv("WAI_NO_COL16", "1")
            assert sim.pc_kernel_name() == ("k_pc_park<spmv>" if not FALLBACK else sim.pc_kernel_name())
            for tag, spmv, composed, split in variants:
                ck.variant("int32 " + tag, spmv, composed, split)
            monkeypatch.delenv("WAI_NO_COL16")
        if case in SLICED and kernel != LEVELS:
            # the comparisons above went through the sliced finalisation: k_finalize's slice loop (-2), the finaliser workgroups
            # with their second-level partial sums (-1 and the drivers' phases)
            nb, nf = SLICED[case]
            ck.apply(dot_mode=3, fin_phase=-1)
            assert sim.partial_count() == (nb if not FALLBACK else len(sub) - 1), (case, sim.partial_count(), nb)
            assert fin_slices(sim.partial_count()) >= nf and (nf < 3 or nb % nf != 0), (case, sim.partial_count(), nf)
        ck.local_input(sub, rp, ci)
        ck.report(kernel)
    sim.destroy()
