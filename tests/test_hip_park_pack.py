"""Short bricks packed into shared k_pc_park workgroups (ilu_schedule.hpp, pack_groups; k_pc_park<.., PACK>), through the C
ABI (wai_test_pc_operator, wai_test_pack_groups), on eos we in 16 x 16 x 2 bricks with the cells in hyperplane order and
random values.

Two comparisons per case: every form of the application (plain, operator, composed operator) with every dot mode and
every way of finishing the sums (k_finalize, in the launch, the drivers' phases) against the long-double reference at
Checker's bars (tests/test_hip_fused_operator.py: z within 1e-12 max|z_ref|, an inner product within 1e-13 sum |a_i b_i|),
and the same runs bit for bit -- z and all 16 scalars -- against WAI_NO_PACK=1, which launches one workgroup per brick on the
same schedule.  Packing moves a brick to other waves of another workgroup and changes nothing it computes, so the bits
must be the same.

Shapes: 24 x 24 x 4 has, per layer pair, one full brick, two half bricks and one quarter brick (8 bricks in 5 workgroups: the
halves in pairs, the two quarters together); 20 x 18 x 5 has members of 16, 64, 128 and 256 rows, so up to eight bricks in
a workgroup and idle waves.  The interior / face split needs a brick that touches no face of the box: 24 x 24 x 4 (two layer pairs) has none --
the library has no lists to split over there and refuses -- so the split runs on 40 x 36 x 6 (3 x 3 x 3 bricks, one
interior), whose face list packs."""
import numpy as np
import pytest

from tests import fused_reference as fr
from tests.test_hip_fused_operator import ALPHA, DRIVER_PHASE, Checker, fd_jacobian
from waiwera_amd.cases import make_case
from waiwera_amd.lib import WaiError

pytestmark = pytest.mark.gpu

BRICK = (16, 16, 2)
PARK = "k_pc_park<spmv,col16>"
SWITCHES = ("WAI_NO_PACK", "WAI_NO_COL16", "WAI_NO_DESC_SHARE")


def structured(dims, brick_order="x"):
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=dims, brick=BRICK, eos="we", lens=True, brick_order=brick_order, order="hyperplane")
    return lm, FlowSimulation(lm, eos="we"), prim, region


def clean(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def applications(sim, n, seed, split=False):
    """z and the 16 scalars of every form of the launch, every dot mode, finished by k_finalize (-2), in the launch (-1) and
    with the drivers' phases"""
    rng = np.random.default_rng(seed)
    x, x2, aux = (fr.spread_vector(n, 2, rng) for _ in range(3))
    s_in = np.zeros(16)
    s_in[fr.S_RHO], s_in[fr.S_RHOOLD], s_in[fr.S_OMEGA], s_in[fr.S_BETA], s_in[fr.S_ALPHA] = 0.83, 1.7, 0.61, 2.3, ALPHA
    out = []
    for spmv, xx2 in ((True, None), (True, x2)) if split else ((False, None), (True, None), (True, x2)):
        for mode in range(5):
            for phase in ((-2,) if mode == 0 else (-2, -1, DRIVER_PHASE[mode])):
                z, s = sim.pc_operator(x, alpha=ALPHA, scal_in=s_in, x2=xx2, dot_mode=mode, aux=aux if mode in (1, 4) else None,
                                       spmv=spmv, fin_phase=phase, split=split)
                out.append(((spmv, xx2 is not None, mode, phase), z, s))
    return out


def same_bits(a, b):
    assert len(a) == len(b)
    for (ka, za, sa), (kb, zb, sb) in zip(a, b):
        assert ka == kb
        assert np.array_equal(za, zb), (ka, np.abs(za - zb).max())
        assert np.array_equal(sa, sb, equal_nan=True), (ka, sa - sb)


def check_table(sim, sub, which=0, bricks=None):
    """the device's group table holds every brick of the list once, on whole waves of its own"""
    ng, shared, tab = sim.pack_groups(which)
    rows = np.diff(sub)
    seen = []
    for g in tab:
        for b in np.unique(g[:, 0][g[:, 0] >= 0]):
            w = np.flatnonzero(g[:, 0] == b)
            assert len(w) == (rows[b] + 63) // 64 and (np.diff(w) == 1).all() and (g[w, 1] == 64 * w[0]).all()
            seen.append(int(b))
    assert sorted(seen) == sorted(range(len(rows)) if bricks is None else bricks)
    return ng, shared, tab


def both_comparisons(sim, lm, monkeypatch, label, seed):
    rp, ci = sim.setup_jacobian()
    sub = np.asarray(lm.sub_ptr)
    n = len(rp) - 1
    val = fr.random_values(rp, ci, 2, np.random.default_rng(seed))
    ck = Checker(sim, rp, ci, sub, 2, val, (label, "packed"))
    ng, shared, tab = check_table(sim, sub)
    print("%s: %d bricks in %d workgroups, %d share theirs, largest group %d" %
          (label, len(sub) - 1, ng, shared, max(len(np.unique(g[:, 0][g[:, 0] >= 0])) for g in tab)))
    assert 0 < ng < len(sub) - 1 and shared > 0               # the packed kernel is what runs
    ck.variant("B^-1 x", False, False, False)
    ck.variant("B^-1 A x", True, False, False)
    ck.variant("B^-1 A (x - a x2)", True, True, False)
    ck.report(sim.pc_kernel_name())
    packed = applications(sim, n, seed + 1)
    monkeypatch.setenv("WAI_NO_PACK", "1")
    assert sim.pack_groups()[0] == 0 and sim.pc_kernel_name() == PARK
    same_bits(packed, applications(sim, n, seed + 1))
    monkeypatch.delenv("WAI_NO_PACK")
    return tab


def test_24x24x4_every_form_and_dot_mode(monkeypatch):
    clean(monkeypatch)
    lm, sim, prim, region = structured((24, 24, 4))
    assert sim.pc_kernel_name() == PARK
    rows = np.diff(np.asarray(lm.sub_ptr))
    assert sorted(rows.tolist()) == [128, 128, 256, 256, 256, 256, 512, 512]
    tab = both_comparisons(sim, lm, monkeypatch, "24x24x4", 31)
    members = sorted(sorted(rows[np.unique(g[:, 0][g[:, 0] >= 0])].tolist()) for g in tab)
    assert members == [[128, 128], [256, 256], [256, 256], [512], [512]]
    # no brick away from the box's faces: no interior / face lists, and the split launch is refused, not answered
    assert sim.pack_groups(1)[0] == 0 and sim.pack_groups(2)[0] == 0
    with pytest.raises(WaiError):
        sim.pc_operator(np.zeros(sim.num_dof), split=True)
    sim.destroy()


@pytest.mark.parametrize("brick_order", ["x", "tile4x4"])
def test_20x18x5_eight_bricks_in_a_workgroup(brick_order, monkeypatch):
    clean(monkeypatch)
    lm, sim, prim, region = structured((20, 18, 5), brick_order)
    assert sim.pc_kernel_name() == PARK
    rows = np.diff(np.asarray(lm.sub_ptr))
    assert {16, 64, 128, 256, 512} <= set(rows.tolist())
    tab = both_comparisons(sim, lm, monkeypatch, "20x18x5 " + brick_order, 33)
    sizes = [len(np.unique(g[:, 0][g[:, 0] >= 0])) for g in tab]
    assert max(sizes) >= 4 and any((g[:, 0] < 0).any() for g in tab)          # several members, and idle waves
    sim.destroy()


def test_bicgstab_solve_same_bits(oracle, monkeypatch):
    """one BiCGStab solve on the FD Jacobian of 24 x 24 x 4: iteration count, reason, residual norm and solution by bit"""
    clean(monkeypatch)
    lm, sim, prim, region = structured((24, 24, 4))
    rp, ci, J = fd_jacobian(oracle, lm, "we", prim, region)
    n = len(rp) - 1
    sim.set_opts(ksp_type="bcgs", ksp_rtol=1e-10)
    sim.set_jacobian_values(J)
    b = np.random.default_rng(35).normal(size=2 * n)
    res = {}
    for tag in ("packed", "own"):
        if tag == "own":
            monkeypatch.setenv("WAI_NO_PACK", "1")
        assert sim.pc_setup() == 0
        assert (sim.pack_groups()[0] > 0) == (tag == "packed")
        x = np.zeros(2 * n)
        its, reason, rn = sim.ksp_solve(b, x)
        res[tag] = (its, reason, rn, x)
    print("BiCGStab: %d iterations, reason %d, residual norm %.3e" % res["packed"][:3])
    assert res["packed"][1] > 0 and res["packed"][0] >= 3
    assert res["packed"][:3] == res["own"][:3]
    assert np.array_equal(res["packed"][3], res["own"][3])
    sim.destroy()


def test_interior_and_face_launches_same_bits(monkeypatch):
    """40 x 36 x 6, every face of the box taken for a partition face (as kernel probes 9 and 10 do): the interior launch and
    the packed face launch give the bits of the unsplit packed launch, and of the unpacked split"""
    clean(monkeypatch)
    lm, sim, prim, region = structured((40, 36, 6))
    assert sim.pc_kernel_name() == PARK
    rp, ci = sim.setup_jacobian()
    sub = np.asarray(lm.sub_ptr)
    n = len(rp) - 1
    sim.set_jacobian_values(fr.random_values(rp, ci, 2, np.random.default_rng(37)))
    assert sim.pc_setup() == 0
    owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
    face = np.zeros(len(sub) - 1, dtype=bool)
    np.logical_or.at(face, owner, np.diff(rp) < 7)
    assert face.any() and not face.all()
    assert sim.pack_groups(1)[0] == 0                              # interior bricks are full bricks: nothing packs
    ng, shared, tab = check_table(sim, sub, 2, np.flatnonzero(face).tolist())
    assert 0 < ng < face.sum() and shared > 0
    whole = [r for r in applications(sim, n, 38) if r[0][0]]       # (the split is the operator's: no plain application)
    split = applications(sim, n, 38, split=True)
    same_bits(whole, split)
    monkeypatch.setenv("WAI_NO_PACK", "1")
    same_bits(split, applications(sim, n, 38, split=True))
    sim.destroy()
