"""The brick's own operand segment staged in LDS (k_pc_park<.., STAGE>, pc_park.hip.h), through the C ABI
(wai_test_pc_operator, wai_ksp_solve), on eos we in 16 x 16 x 2 bricks with the cells in hyperplane order and random values.

WAI_PARK_STAGE=1 makes every operator launch of k_pc_park on its 16-bit column indices store S_i = R_i - alpha V_i (or its
one operand vector's entry) to the idle solution area and read the in-brick columns' entries from there; =0 gathers them
from memory as before.  An entry read from LDS was formed by the same fma from the same two doubles as the gathered one, the
products and their order are the same, so z and all 16 scalars must be the same bits.  Each case runs every form of the
operator -- plain, composed, and both over the one-rank interior / face launch lists -- with every dot mode (ZA and the
merged five among them) and every way of finishing the sums, staged against the long-double reference at Checker's bars
(tests/test_hip_fused_operator.py: z within 1e-12 max|z_ref|, an inner product within 1e-13 sum |a_i b_i|), and staged
against unstaged bit for bit.

Shapes: 48 x 48 x 6 is 3 x 3 x 3 full bricks, one of them interior, the others on every combination of the box's faces
(nothing packs: one workgroup per brick); 40 x 40 x 6 splits as 16 + 16 + 8 in x and y, so the ragged bricks share
workgroups (k_pc_park<.., PACK, STAGE>: members at a thread offset, waves without a brick)."""
import numpy as np
import pytest

from tests import fused_reference as fr
from tests.test_hip_fused_operator import Checker, fd_jacobian
from tests.test_hip_park_pack import PARK, SWITCHES, applications, same_bits, structured

pytestmark = pytest.mark.gpu

STAGE = "WAI_PARK_STAGE"


def clean(monkeypatch):
    for k in SWITCHES + (STAGE,):
        monkeypatch.delenv(k, raising=False)


def off_on_reference(dims, monkeypatch, seed, packed):
    clean(monkeypatch)
    lm, sim, prim, region = structured(dims)
    assert sim.pc_kernel_name() == PARK
    rp, ci = sim.setup_jacobian()
    sub = np.asarray(lm.sub_ptr)
    n = len(rp) - 1
    assert len(sub) - 1 == 27
    owner = np.repeat(np.arange(27), np.diff(sub))
    face = np.zeros(27, dtype=bool)
    np.logical_or.at(face, owner, np.diff(rp) < 7)
    assert (~face).sum() == 1                                   # one brick away from every face of the box
    val = fr.random_values(rp, ci, 2, np.random.default_rng(seed))
    monkeypatch.setenv(STAGE, "1")
    ck = Checker(sim, rp, ci, sub, 2, val, ("%dx%dx%d" % dims, "staged"))
    ng = [sim.pack_groups(w)[0] for w in range(3)]
    assert (ng[0] > 0 and ng[2] > 0) == packed, ng              # 40 x 40 x 6: the whole list and the face list pack
    ck.variant("B^-1 A x", True, False, False)
    ck.variant("B^-1 A (x - a x2)", True, True, False)
    ck.variant("split", True, False, True)
    ck.variant("split composed", True, True, True)
    ck.report(sim.pc_kernel_name())
    on = applications(sim, n, seed + 1) + applications(sim, n, seed + 1, split=True)
    monkeypatch.setenv(STAGE, "0")
    off = applications(sim, n, seed + 1) + applications(sim, n, seed + 1, split=True)
    same_bits(off, on)
    assert any(np.abs(z).max() > 0 for _, z, _ in on)
    sim.destroy()


def test_48x48x6_every_face_combination(monkeypatch):
    off_on_reference((48, 48, 6), monkeypatch, 41, packed=False)


def test_40x40x6_ragged_bricks_in_shared_workgroups(monkeypatch):
    off_on_reference((40, 40, 6), monkeypatch, 43, packed=True)


def test_bicgstab_solve_same_bits(oracle, monkeypatch):
    """one BiCGStab solve on the FD Jacobian of 48 x 48 x 6: iterates, iteration count, reason and the posted residual norm
    by bit, staged against unstaged"""
    clean(monkeypatch)
    lm, sim, prim, region = structured((48, 48, 6))
    rp, ci, J = fd_jacobian(oracle, lm, "we", prim, region)
    n = len(rp) - 1
    sim.set_opts(ksp_type="bcgs", ksp_rtol=1e-10)
    sim.set_jacobian_values(J)
    b = np.random.default_rng(45).normal(size=2 * n)
    res = {}
    for tag in ("0", "1"):
        monkeypatch.setenv(STAGE, tag)
        assert sim.pc_setup() == 0
        x = np.zeros(2 * n)
        its, reason, rn = sim.ksp_solve(b, x)
        res[tag] = (its, reason, rn, x)
    print("BiCGStab: %d iterations, reason %d, residual norm %.3e" % res["1"][:3])
    assert res["1"][1] > 0 and res["1"][0] >= 3
    assert res["0"][:3] == res["1"][:3]
    assert np.array_equal(res["0"][3], res["1"][3])
    sim.destroy()
