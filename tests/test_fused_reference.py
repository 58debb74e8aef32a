"""The long-double reference of tests/fused_reference.py checked on its own, before any GPU comparison relies on it:
the ILU(0) property L U = A on the pattern, agreement with the oracle's block-Jacobi ILU(0), and the exact inverse where
ILU(0) drops nothing."""
import numpy as np
import pytest

from oracle import binding as ol
from tests import fused_reference as fr
from waiwera_amd.cases import make_case

KIND = {"w": 0, "we": 1, "wce": 2, "wsce": 5}


def pattern(oracle, eos, lm):
    osim = ol.OracleSim(oracle, lm, KIND[eos])
    rp, ci = osim.pattern()
    osim.close()
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int32)


def meshes():
    # hexahedral bricks (ragged in y and z), MINC bricks (fracture rows, then matrix rows), the triangle mesh
    yield "hex", "we", make_case(dims=(7, 6, 5), brick=(4, 4, 2), eos="we")[1]
    yield "minc", "wce", make_case(dims=(6, 4, 3), brick=(4, 4, 2), eos="wce", minc=True)[1]
    yield "triangles", "we", fr.triangle_mesh("we")[1]


@pytest.mark.parametrize("which", ["hex", "minc", "triangles"])
def test_lu_equals_a_on_the_pattern(oracle, which):
    name, eos, lm = next(m for m in meshes() if m[0] == which)
    rp, ci, sub = pattern(oracle, eos, lm)
    bs = {"we": 2, "wce": 3}[eos]
    val = fr.random_values(rp, ci, bs, np.random.default_rng(5))
    f = fr.BlockILU0(rp, ci, val, bs, sub)
    assert f.offdiag_updates == (which == "triangles")   # only a cell graph with triangles has off-diagonal fill
    L, U = f.L_blocks()
    A = np.asarray(val, dtype=fr.LD).reshape(-1, bs, bs)
    n = len(rp) - 1
    worst = 0.0
    for i in range(n):
        for q in range(rp[i], rp[i + 1]):
            j = int(ci[q])
            if (i, j) not in L and (i, j) not in U:
                continue   # the coupling leaves the subdomain
            m = min(i, j)
            acc = np.zeros((bs, bs), dtype=fr.LD)
            for k, _ in f.lower[i]:
                if k < m and (k, j) in U:
                    acc += L[(i, k)] @ U[(k, j)]
            acc += L[(i, j)] @ U[(j, j)] if j < i else U[(i, j)]
            worst = max(worst, float(np.abs(acc - A[q]).max() / np.abs(A[q]).max()))
    print(which, "max |(LU)_ij - A_ij| / |A_ij| on the pattern:", worst)
    assert worst < 1e-16


@pytest.mark.parametrize("which", ["hex", "minc", "triangles"])
def test_matches_the_oracle_bilu0(oracle, which):
    name, eos, lm = next(m for m in meshes() if m[0] == which)
    rp, ci, sub = pattern(oracle, eos, lm)
    bs = {"we": 2, "wce": 3}[eos]
    n = len(rp) - 1
    rng = np.random.default_rng(6)
    val = fr.random_values(rp, ci, bs, rng)
    fval, dinv = np.zeros_like(val), np.zeros(n * bs * bs)
    assert oracle.wo_bilu0_factor(n, bs, ol.ip(rp), ol.ip(ci), ol.dp(val), len(sub) - 1, ol.ip(sub), ol.dp(fval), ol.dp(dinv)) == 0
    r = fr.spread_vector(n, bs, rng)
    zo = np.zeros(n * bs)
    oracle.wo_bilu0_apply(n, bs, ol.ip(rp), ol.ip(ci), ol.dp(fval), ol.dp(dinv), len(sub) - 1, ol.ip(sub), ol.dp(r), ol.dp(zo))
    z = fr.BlockILU0(rp, ci, val, bs, sub).solve(r)
    err = float(np.abs(z - zo).max() / np.abs(z).max())
    print(which, "reference against wo_bilu0_apply:", err)
    assert err < 1e-12


@pytest.mark.parametrize("bs", [1, 2, 3, 4])
def test_exact_inverse_on_a_chain(bs):
    """a single subdomain whose cell graph is a chain: ILU(0) drops nothing, B^-1 is the dense inverse"""
    n = 17
    rp, ci = [0], []
    for i in range(n):
        ci += [j for j in (i - 1, i, i + 1) if 0 <= j < n]
        rp.append(len(ci))
    rp, ci = np.array(rp, dtype=np.int32), np.array(ci, dtype=np.int32)
    rng = np.random.default_rng(7 + bs)
    val = fr.random_values(rp, ci, bs, rng)
    f = fr.BlockILU0(rp, ci, val, bs, [0, n])
    dense = np.zeros((n * bs, n * bs))
    V = val.reshape(-1, bs, bs)
    for i in range(n):
        for q in range(rp[i], rp[i + 1]):
            dense[i * bs:(i + 1) * bs, ci[q] * bs:(ci[q] + 1) * bs] = V[q]
    Binv = np.column_stack([f.solve(e).astype(np.float64) for e in np.eye(n * bs)])
    err = np.abs(Binv - np.linalg.inv(dense)).max() / np.abs(Binv).max()
    assert err < 1e-13, err
    # and the operator B^-1 A is the identity
    x = fr.spread_vector(n, bs, rng)
    assert np.abs(f.operator(val, x).astype(np.float64) - x).max() < 1e-13 * np.abs(x).max()


def test_block_inverse_in_long_double():
    rng = np.random.default_rng(8)
    B = rng.normal(size=(50, 4, 4)).astype(fr.LD)
    B[:, 0, 0] = 0.0   # a zero leading entry: the pivot search must swap
    Bi = fr.inv_blocks(B)
    err = np.abs(np.matmul(B, Bi) - np.eye(4, dtype=fr.LD)).max()
    assert err < 1e-16 * np.abs(B).max() * np.abs(Bi).max() * 40


def test_derived_scalars_compose():
    """phase 6 is phase 5 then the rotation of phase 4; phase 2 / 3 are the two quotients"""
    s = np.arange(16, dtype=float) * 0.37 + 1.0
    s[fr.S_BREAK] = 0.0
    s6, _ = fr.derive(s, 6)
    s5, _ = fr.derive(s, 5)
    s54, _ = fr.derive(s5, 4)
    assert np.array_equal(s6, s54)
    assert fr.derive(s, 2)[0][fr.S_ALPHA] == s[fr.S_RHO] / s[fr.S_D1]
    assert fr.derive(s, 3)[0][fr.S_OMEGA] == s[fr.S_D1] / s[fr.S_D2]
