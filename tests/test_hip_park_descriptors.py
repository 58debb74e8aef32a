"""k_pc_park's two descriptor changes, through the C ABI (wai_test_pc_operator), on eos we in 16 x 16 x 2 bricks with the
cells in hyperplane order and random operands:

* the row's own operand entry for the inner products comes from the diagonal slot's gather (SPMV) or from the row's
  pivot-scaled input (plain application), no longer from a load of its own;
* on the 16-bit column indices the per-row descriptors (row_info, row_uoff, the col16 record) are read from one copy per
  distinct brick (IluSchedule::t_*, sub_desc); WAI_NO_DESC_SHARE reads every brick's own through the same kernel.

Bars are Checker's (tests/test_hip_fused_operator.py): z within 1e-12 max|z_ref|, an inner product within 1e-13
sum |a_i b_i| of the long-double reference.  Checker.variant runs every dot mode -- ZA (1), XZ (2), ZZ (3), merged (4) --
with the sums finished by k_finalize, in the launch, and with the drivers' phases.

Template counts: a full brick's descriptors depend on which faces of the box it touches (a missing neighbour is a
padding slot and moves the diagonal's slot), so a box of bx x by x bz bricks has at most
min(bx, 3) * min(by, 3) * min(bz, 3) classes of full bricks: 27 of the 48 bricks of 64 x 64 x 6.  The 18 bricks of
48 x 48 x 4 (3 x 3 x 2) each touch a different set of faces, so that mesh has 18 templates and the count is shown to
fall below the brick count on 64 x 64 x 6."""
import os

import numpy as np
import pytest

from tests import fused_reference as fr
from tests.test_hip_fused_operator import Checker
from waiwera_amd.cases import make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRICK = (16, 16, 2)
PARK = "k_pc_park<spmv,col16>"


def structured(dims, brick_order="x"):
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=dims, brick=BRICK, eos="we", lens=True, brick_order=brick_order, order="hyperplane")
    return lm, FlowSimulation(lm, eos="we")


def unstructured_fixture():
    """the reference's problem-5 gmsh mesh (96 cells, 2-D), subdomains = chunks of 16 consecutive cells"""
    from waiwera_amd import gmsh, unstructured
    from waiwera_amd.flow_simulation import FlowSimulation
    nodes, cells, dim = gmsh.read_msh(os.path.join(ROOT, "tests", "golden", "inputs", "gproblem5.msh"))
    rock = np.array([2.5e-14, 2.5e-14, 2.5e-14, 1.0, 1.0, 0.35, 2500.0, 1000.0])
    lm = unstructured.build_mesh(nodes, cells, dim, thickness=100.0, rock=rock, chunk=16)
    return lm, FlowSimulation(lm, eos="we")


def applications(sim, n, rng):
    """z and the 16 scalars of every form of the launch: plain application, operator, composed operator; all dot modes"""
    bs = 2
    x, x2, aux = (fr.spread_vector(n, bs, rng) for _ in range(3))
    s_in = np.zeros(16)
    s_in[fr.S_RHO], s_in[fr.S_RHOOLD], s_in[fr.S_OMEGA], s_in[fr.S_BETA], s_in[fr.S_ALPHA] = 0.83, 1.7, 0.61, 2.3, 0.37
    out = []
    for spmv, xx2 in ((False, None), (True, None), (True, x2)):
        for mode in range(5):
            for phase in ((-2,) if mode == 0 else (-2, -1)):
                z, s = sim.pc_operator(x, alpha=0.37, scal_in=s_in, x2=xx2, dot_mode=mode, aux=aux if mode in (1, 4) else None,
                                       spmv=spmv, fin_phase=phase)
                out.append(((spmv, xx2 is not None, mode, phase), z, s))
    return out


def same_bits(a, b):
    assert len(a) == len(b)
    for (ka, za, sa), (kb, zb, sb) in zip(a, b):
        assert ka == kb
        assert np.array_equal(za, zb), (ka, np.abs(za - zb).max())
        assert np.array_equal(sa, sb, equal_nan=True), (ka, sa - sb)


def prepared(sim, seed):
    rp, ci = sim.setup_jacobian()
    sim.set_jacobian_values(fr.random_values(rp, ci, 2, np.random.default_rng(seed)))
    assert sim.pc_setup() == 0
    return len(rp) - 1


@pytest.mark.parametrize("brick_order", ["x", "tile4x4"])
def test_ragged_bricks_against_long_double_reference(brick_order, monkeypatch):
    """20 x 18 x 5: bricks ragged on every axis (16 + 4, 16 + 2, 2 + 2 + 1), so threads beyond a brick's rows; rows whose
    diagonal is slot 0 and rows whose diagonal is the last slot; boundary rows with padding slots."""
    monkeypatch.delenv("WAI_NO_COL16", raising=False)
    monkeypatch.delenv("WAI_NO_DESC_SHARE", raising=False)
    lm, sim = structured((20, 18, 5), brick_order)
    assert sim.pc_kernel_name() == PARK
    rp, ci = sim.setup_jacobian()
    sub = np.asarray(lm.sub_ptr)
    n = len(rp) - 1
    width = np.diff(rp)
    rows = np.repeat(np.arange(n), width)
    dpos = np.flatnonzero(ci == rows) - rp[:-1]          # the diagonal's slot
    assert len(dpos) == n and width.max() == 7
    assert (dpos == 0).any() and (dpos == width - 1).any() and (width < 7).any()
    assert len(sub) - 1 == 2 * 2 * 3 and len(set(np.diff(sub).tolist())) > 4 and np.diff(sub).max() == 512
    val = fr.random_values(rp, ci, 2, np.random.default_rng(21))
    for share in (True, False):
        if not share:
            monkeypatch.setenv("WAI_NO_DESC_SHARE", "1")
        ck = Checker(sim, rp, ci, sub, 2, val, ("20x18x5 " + brick_order, "shared" if share else "own"))
        ck.variant("B^-1 x", False, False, False)
        ck.variant("B^-1 A x", True, False, False)
        ck.variant("B^-1 A (x - a x2)", True, True, False)
        ck.report(sim.pc_kernel_name())
    sim.destroy()


@pytest.fixture(scope="module")
def box48():
    lm, sim = structured((48, 48, 4))
    n = prepared(sim, 22)
    yield lm, sim, n
    sim.destroy()


def test_shared_descriptors_same_bits_48x48x4(box48, monkeypatch):
    """z and the sums, every form and dot mode: the templates against every brick's own descriptors (WAI_NO_DESC_SHARE)
    and against the int32 column planes (WAI_NO_COL16)"""
    monkeypatch.delenv("WAI_NO_COL16", raising=False)
    monkeypatch.delenv("WAI_NO_DESC_SHARE", raising=False)
    lm, sim, n = box48
    assert sim.pc_kernel_name() == PARK
    shared = applications(sim, n, np.random.default_rng(23))
    monkeypatch.setenv("WAI_NO_DESC_SHARE", "1")
    same_bits(shared, applications(sim, n, np.random.default_rng(23)))
    monkeypatch.delenv("WAI_NO_DESC_SHARE")
    monkeypatch.setenv("WAI_NO_COL16", "1")
    assert sim.pc_kernel_name() == "k_pc_park<spmv>"
    same_bits(shared, applications(sim, n, np.random.default_rng(23)))


def test_template_count_48x48x4(box48):
    """48 x 48 x 4 is 3 x 3 x 2 full bricks, and each of the 18 touches a different set of the box's faces (x: lower,
    none, upper; y likewise; z: lower or upper), so no two have the same descriptors: 18 templates, one per brick, each
    brick's rows stored once.  (The count falls below the brick count once a class of bricks repeats: the next test.)"""
    nt, nb, nr = box48[1].desc_templates()
    print("48 x 48 x 4: %d templates (%d rows, %d bytes) for %d bricks" % (nt, nr, 24 * nr, nb))
    assert (nt, nb, nr) == (18, 18, 9216)


def test_templates_of_a_box_with_interior_bricks(monkeypatch):
    """64 x 64 x 6 = 4 x 4 x 3 full bricks: three classes per axis (lower face, interior, upper face), 27 templates for 48
    bricks at the most (MEASURED: 27); same bits with and without the sharing"""
    monkeypatch.delenv("WAI_NO_COL16", raising=False)
    monkeypatch.delenv("WAI_NO_DESC_SHARE", raising=False)
    lm, sim = structured((64, 64, 6))
    assert sim.pc_kernel_name() == PARK
    n = prepared(sim, 24)
    nt, nb, nr = sim.desc_templates()
    print("64 x 64 x 6: %d templates (%d rows, %d bytes) for %d bricks" % (nt, nr, 24 * nr, nb))
    assert nb == 48 and 0 < nt <= 27 and nt < nb and nr == 512 * nt, (nt, nb, nr)
    shared = applications(sim, n, np.random.default_rng(25))
    monkeypatch.setenv("WAI_NO_DESC_SHARE", "1")
    same_bits(shared, applications(sim, n, np.random.default_rng(25)))
    sim.destroy()


def test_unstructured_mesh_same_bits(monkeypatch):
    """a gmsh mesh cut into chunks of consecutive cells: nothing is shared but what is byte-identical (MEASURED: two of the six
    chunks of this mesh of regular quadrilaterals are, 5 templates of 80 rows), and the results keep their bits"""
    monkeypatch.delenv("WAI_NO_COL16", raising=False)
    monkeypatch.delenv("WAI_NO_DESC_SHARE", raising=False)
    lm, sim = unstructured_fixture()
    assert sim.pc_kernel_name() == PARK
    n = prepared(sim, 26)
    nt, nb, nr = sim.desc_templates()
    print("gproblem5.msh: %d templates (%d rows) for %d chunks of %d rows" % (nt, nr, nb, n))
    assert (nt, nb, nr) == (5, 6, 80)
    shared = applications(sim, n, np.random.default_rng(27))
    monkeypatch.setenv("WAI_NO_DESC_SHARE", "1")
    same_bits(shared, applications(sim, n, np.random.default_rng(27)))
    monkeypatch.delenv("WAI_NO_DESC_SHARE")
    monkeypatch.setenv("WAI_NO_COL16", "1")
    same_bits(shared, applications(sim, n, np.random.default_rng(27)))
    sim.destroy()
