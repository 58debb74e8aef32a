"""The multicolour reference (tests/colour_reference.py) against ILU(0)'s defining property, without a GPU: on every pattern
entry inside a subdomain (L U)_ij = A_ij, where L (unit diagonal) and U are the factor's blocks in elimination order."""
import numpy as np
import pytest

from tests import colour_reference as cr
from tests import fused_reference as fr
from waiwera_amd.cases import make_case

pattern = cr.mesh_pattern

LD = fr.LD
EPS = np.finfo(LD).eps


def box_case():
    g, lm, prim, region = make_case(dims=(6, 6, 4), brick=(3, 3, 2), eos="we")
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), 2


def triangle_case():
    g, lm, prim, region = fr.triangle_mesh()
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), 3


def one_block_case():
    rp, ci, sub, bs = box_case()
    return rp, ci, np.array([0, len(rp) - 1]), 1


@pytest.mark.parametrize("make", [box_case, triangle_case, one_block_case])
def test_lu_equals_a_on_the_pattern(make):
    """Entry (i, j): A_ij - sum_k L_ik U_kj is what the elimination left of a block after at most 15 subtractions of a
    product of bs terms, each rounded once in long double: the bar is 4 ulps per rounded term of the entry's scale
    |A_ij| + sum_k |L_ik| |U_kj| (max norms times bs for the products)."""
    rp, ci, sub, bs = make()
    rng = np.random.default_rng(5)
    val = fr.random_values(rp, ci, bs, rng)
    ref = cr.ColourILU0(rp, ci, val, bs, sub)
    n = ref.n
    V = np.asarray(val, dtype=LD).reshape(-1, bs, bs)
    F = ref.factor_blocks()
    key = ref.colour * n + np.arange(n)          # elimination order
    owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
    nbrs = [[int(j) for j in ci[rp[i]:rp[i + 1]] if j < n and owner[j] == owner[i]] for i in range(n)]
    checked = 0
    for i in range(n):
        for q in range(rp[i], rp[i + 1]):
            j = int(ci[q])
            if j >= n or owner[j] != owner[i]:
                continue
            acc = np.zeros((bs, bs), dtype=LD)
            scale = np.abs(V[q]).max()
            terms = 1
            for k in nbrs[i]:
                if key[k] < key[i] and key[k] <= key[j] and (k == j or (k, j) in F):
                    acc += F[(i, k)] @ F[(k, j)]
                    scale += bs * np.abs(F[(i, k)]).max() * np.abs(F[(k, j)]).max()
                    terms += bs
            if key[i] <= key[j]:
                acc += F[(i, j)]                 # the unit diagonal of L times U_ij
                scale += np.abs(F[(i, j)]).max()
            err = np.abs(acc - V[q]).max()
            assert err <= 4 * terms * EPS * scale, (i, j, float(err), float(scale))
            checked += 1
    assert checked > n
    assert ref.offdiag_updates == (make is triangle_case)


def test_two_colours_on_the_box_and_three_on_triangles():
    rp, ci, sub, bs = box_case()
    assert cr.greedy_colours(rp, ci, sub).max() == 1
    rp, ci, sub, bs = triangle_case()
    assert cr.greedy_colours(rp, ci, sub).max() >= 2


def test_permutation_sorts_by_colour_then_row():
    rp, ci, sub, bs = box_case()
    colour = cr.greedy_colours(rp, ci, sub)
    new = cr.permutation(colour, sub)
    for s in range(len(sub) - 1):
        rows = np.arange(sub[s], sub[s + 1])
        assert sorted(new[rows]) == rows.tolist()
        order = rows[np.argsort(new[rows])]
        keys = [(colour[i], i) for i in order]
        assert keys == sorted(keys)


def test_one_colour_system_is_exact():
    """a block-diagonal system has one colour and the factor is the diagonal: with blocks 2^k I and integer data, r = D x
    is exact and so is z = D^-1 r"""
    n, bs = 7, 2
    rp, ci = np.arange(n + 1), np.arange(n)
    rng = np.random.default_rng(2)
    scale = 2.0 ** rng.integers(-3, 4, size=n)
    val = (scale[:, None, None] * np.eye(bs)[None]).ravel()
    ref = cr.ColourILU0(rp, ci, val, bs, np.array([0, 3, n]))
    assert ref.colour.max() == 0
    x = rng.integers(-50, 50, size=n * bs).astype(np.float64)
    r = fr.spmv(rp, ci, val, bs, x)
    assert np.array_equal(ref.solve(r), x.astype(LD)) and np.array_equal(ref.operator(val, x), x.astype(LD))
