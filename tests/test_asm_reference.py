"""The pure-Python PCASM reference of tests/asm_reference.py, checked on the CPU: the block sizes and widths the fused
launch's conditions rest on (an extended block of at most 1024 rows, a row of E of at most 16 blocks), and the reference
itself against dense restricted additive Schwarz where ILU(0) is exact."""
import numpy as np
import pytest

from tests import asm_reference as ar
from waiwera_amd.cases import make_case


def case_pattern(key):
    eos, dims, brick, overlap, levels = key
    # (imported here, not at the top: that module loads the HIP library, and collecting this file must not do so ahead of
    # the modules that import torch -- torch's own HIP runtime has to be the process's first)
    from tests.test_hip_iluk_fused import mesh_pattern
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=(eos == "we"))
    rp, ci = mesh_pattern(lm)
    return lm, ar.AsmPattern(rp, ci, np.asarray(lm.sub_ptr), overlap, levels)


@pytest.mark.parametrize("case", list(ar.CASES))
def test_fused_cases_fit_a_workgroup_and_the_wide_descriptor(case):
    lm, pat = case_pattern(ar.CASES[case])
    print(case, "largest extended block", pat.max_rows, "rows; widest row of E", pat.width, "blocks")
    assert pat.max_rows <= 1024 and pat.width <= 16
    assert pat.max_rows > np.diff(lm.sub_ptr).max()          # the overlap is real
    if case == "we_full_block":
        assert pat.max_rows == ar.interior_rows(16, 14, 2) == 1016
    if case == "we_ilu1":
        assert pat.width > 7                                  # and so is the fill


def test_the_bench_brick_is_too_big():
    lm, pat = case_pattern(ar.TOO_BIG)
    assert pat.max_rows == ar.interior_rows(16, 16, 2) == 1152 > 1024
    assert ar.interior_rows(15, 15, 2) == 1020


@pytest.mark.parametrize("overlap", [1, 2])
def test_reference_is_restricted_additive_schwarz(overlap):
    """a chain of 12 block rows in three blocks: ILU(0) of a block tridiagonal matrix is its LU, so the reference must equal
    dense restricted additive Schwarz, z = sum_b R~_b^T (R_b A R_b^T)^-1 R_b r"""
    n, bs = 12, 2
    sub = np.array([0, 4, 8, 12])
    cols = [[j for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)]
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(c) for c in cols])
    ci = np.array([j for c in cols for j in c], dtype=np.int64)
    rng = np.random.default_rng(3)
    from tests import fused_reference as fr
    val = fr.random_values(rp, ci, bs, rng)
    pat = ar.AsmPattern(rp, ci, sub, overlap)
    want = [(max(sub[b] - overlap, 0), min(sub[b + 1] + overlap, n)) for b in range(3)]
    assert [(int(pat.ext_row[pat.ext_ptr[b]]), int(pat.ext_row[pat.ext_ptr[b + 1] - 1]) + 1) for b in range(3)] == want
    A = np.zeros((n * bs, n * bs))
    V = val.reshape(-1, bs, bs)
    for i in range(n):
        for q in range(rp[i], rp[i + 1]):
            A[i * bs:(i + 1) * bs, ci[q] * bs:(ci[q] + 1) * bs] = V[q]
    r = rng.normal(size=n * bs)
    z = np.zeros(n * bs)
    for b, (lo, hi) in enumerate(want):
        s = slice(lo * bs, hi * bs)
        zb = np.linalg.solve(A[s, s], r[s])
        own = slice((sub[b] - lo) * bs, (sub[b + 1] - lo) * bs)
        z[sub[b] * bs:sub[b + 1] * bs] = zb[own]
    ref = ar.AsmRef(pat, val, bs)
    got = ref.solve(r).astype(np.float64)
    assert np.abs(got - z).max() <= 1e-12 * np.abs(z).max()
    x = rng.normal(size=n * bs)
    assert np.abs(ref.operator(val, x).astype(np.float64) - ref.solve(A @ x).astype(np.float64)).max() <= 1e-12 * np.abs(z).max()
