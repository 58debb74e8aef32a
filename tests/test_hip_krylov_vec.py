"""The Krylov drivers' vector and reduction launches, one at a time, against the long-double reference of
tests/krylov_vec_reference.py (wai_test_krylov_vec: the drivers' own launchers on temporaries of the test's lengths).

Sizes follow the code: 256 threads per workgroup, a grid capped at 1024 workgroups (a thread strides from n = 262145),
16-byte lanes (odd n: a tail element; odd n with ld = n: every second basis vector only 8-byte aligned), k_mdot's two pairs
per trip (n / 2 > 262144; at 1572867 the paired loop, a second trip, the single remainder and the odd tail together), each
k_mdot<1..8> with the later passes at j0 = 8, 16, ..., k_maxpy_norm's groups of eight with remainders.

Bars (derived, not measured): an element of an updated vector within c 2^-53 M_i of the reference, M_i the sum of the
magnitudes of the terms of its expression, c = 8 for the BiCGStab updates, k_waxpy and k_scale_to (at most five roundings),
c = 2 (k + 2) for k_maxpy_norm and k_update_x (k + 1 roundings); an inner product within 1e-13 sum |a_i b_i|; a derived
scalar within 1e-12 of the restated formula applied to the launch's own sums, relative to the sum of the magnitudes of the
formula's terms; whatever a launch does not write -- scalars, guard elements, the vectors it only reads -- bit for bit
what went in; the posted (R,R) and code bit for bit the device scalars; every op three times bit for bit; and the kernels'
bit-identity claims (k_bcgs_xrp against the three kernels it replaces, its DERIVE form against k_bcgs_scalars(6) in
front of it, the in-launch finalisation against k_finalize).

MEASURED (MI355X; the module prints them): the largest inner-product error is 0.0030 of its bar (3.0e-16 sum |a_i b_i|;
k_mdot 0.0013, k_maxpy_norm's |w|^2 0.0022, k_bcgs_xr's (R,R) 0.0020); the largest element-wise error 0.40 of its bar
(k_maxpy_norm 0.23, k_update_x 0.17 of theirs); the largest derived-scalar error 0.00022 of its bar (2.2e-16 of the terms).
GMRES end to end (12 x 10 x 9 cells, eos we), |estimate - true| / |B^-1 b|: device 2.6e-16, oracle 3.9e-16 and 1.6e-17 by
its OpenMP team size (test_gmres_estimate_is_honest)."""
import numpy as np
import pytest

from tests import krylov_vec_reference as kr
from waiwera_amd.lib import WaiError, device_memory

pytestmark = pytest.mark.gpu

LD = kr.LD
X, R, RP, P, V, S, T = range(7)
SENT = 7.0e77                 # guard elements: behind n in every vector, between and behind the basis vectors
SMALL = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 1023]
BIG = [262143, 262144, 262145]
BIG2 = BIG + [524287, 524289, 1572867]     # the two-entry kernels
K_SMALL = list(range(1, 18)) + [24, 30, 40]
K_BIG = [8, 9]
ALPHA = 0.37
WORST = {"dot": 0.0, "elem": 0.0, "scal": 0.0}


def classes(big):
    return [pytest.param(SMALL, id="small")] + [pytest.param([n], id=str(n)) for n in big]


@pytest.fixture(scope="module")
def sim():
    from waiwera_amd.cases import make_case
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(8, 8, 4), brick=(4, 4, 4), eos="w", lens=False)
    s = FlowSimulation(lm, eos="w")
    yield s
    print("\nlargest inner-product error / bar %.3g, element / bar %.3g, derived scalar / bar %.3g"
          % (WORST["dot"], WORST["elem"], WORST["scal"]))
    s.destroy()


def signed(rng, size):
    """magnitudes 0.1 .. 3, both signs"""
    return rng.uniform(0.1, 3.0, size=size) * rng.choice([-1.0, 1.0], size=size)


def scalars(rng):
    s = signed(rng, kr.NSCAL)
    s[kr.S_BREAK] = 0.0
    return s


def vectors(rng, n, pad=5):
    v = np.full((7, n + pad), SENT)
    v[:, :n] = rng.normal(size=(7, n))
    return v


def cancelling(rng, a):
    """a partner of a whose product with it cancels to near zero: the same entries within 10 %, the first half negated"""
    b = a * rng.uniform(0.9, 1.1, size=a.size)
    b[: a.size // 2] *= -1.0
    return b


def make_basis(rng, n, ldim, k, w=None):
    b = np.full((k + 1, ldim), SENT)
    b[:k, :n] = rng.normal(size=(k, n))
    if w is not None and n > 1023:
        b[0, :n] = cancelling(rng, w[:n])
    return b.ravel()


def same(a, b):
    """bit for bit (tobytes(); the long vectors as 64-bit integers, which compares the same bits without two copies)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.size < 100000:
        return a.tobytes() == b.tobytes()
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def check_elem(got, ref, M, c, what):
    err = np.abs(ld_(got) - ref) / np.maximum(LD(c) * LD(kr.U) * M, LD(1e-300))
    ratio = float(err.max())
    WORST["elem"] = max(WORST["elem"], ratio)
    assert ratio <= 1.0, (what, ratio, int(np.argmax(err)))


def ld_(a):
    return np.asarray(a, dtype=LD)


def check_dot(got, a, b, what):
    d, bar = kr.dot(a, b)
    err = abs(LD(got) - d) / (LD(1e-13) * bar) if bar > 0 else (0.0 if got == 0.0 else np.inf)
    WORST["dot"] = max(WORST["dot"], float(err))
    assert err <= 1.0, (what, got, float(d), float(bar), float(err))
    return float(err)


def check_untouched(vin, vout, sin, sout, n, vec_written=(), scal_written=(), what=""):
    """every vector entry outside the first n of the written vectors, and every scalar outside scal_written: the bits that went in"""
    for i in range(7):
        lo = n if i in vec_written else 0
        assert same(vin[i, lo:], vout[i, lo:]), (what, "vector", i, "guards" if lo else "read-only input")
    keep = [i for i in range(kr.NSCAL) if i not in set(scal_written)]
    assert same(sin[keep], sout[keep]), (what, "scalars", [i for i in keep if not same(sin[i], sout[i])])


def check_basis_untouched(bin_, bout, what):
    assert same(bin_, bout), (what, "basis")


def check_scalars(sout, sin, phase, what):
    """derived scalars against the restated formula applied to sin (which holds the launch's own sums)"""
    want, scale = kr.derive(sin, phase)
    for i in range(kr.NSCAL):
        if scale.get(i, 0.0) > 0.0 and np.isfinite(want[i]):
            err = abs(sout[i] - want[i]) / (1e-12 * scale[i])
            WORST["scal"] = max(WORST["scal"], float(err))
            assert err <= 1.0, (what, phase, i, sout[i], want[i])
        else:   # a constant, a copy, a breakdown code, an infinity or NaN, or a slot the phase does not write
            assert sout[i] == want[i] or (np.isnan(sout[i]) and np.isnan(want[i])), (what, phase, i, sout[i], want[i])
    return want


def thrice(sim, op, n, vin, sin, times=3, **kw):
    """the op three times on the same inputs: bit for bit; the first result"""
    runs = [sim.krylov_vec(op, n, vin, sin, **kw) for _ in range(times)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert (a is None and b is None) or same(a, b), (op, n, kw.get("variant"), "not repeatable")
    return runs[0]


# ---- inner products ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", classes(BIG))
def test_dot_and_dots(sim, sizes):
    for n in sizes:
        rng = np.random.default_rng(1000 + n)
        vin, sin = vectors(rng, n), scalars(rng)
        if n > 1023:
            vin[R, :n] = cancelling(rng, vin[X, :n])
        v, _, s, post = thrice(sim, "dot", n, vin, sin)
        e = check_dot(s[kr.S_W2], vin[X, :n], vin[R, :n], ("dot", n))
        check_untouched(vin, v, sin, s, n, scal_written=[kr.S_W2], what=("dot", n))
        assert np.isnan(post).all()
        v, _, s2, _ = thrice(sim, "dots", n, vin, sin, variant=0)
        check_dot(s2[kr.S_D1], vin[X, :n], vin[R, :n], ("dots", n))
        e2 = check_dot(s2[kr.S_D2], vin[P, :n], vin[V, :n], ("dots", n))
        check_untouched(vin, v, sin, s2, n, scal_written=[kr.S_D1, kr.S_D2], what=("dots", n))
        v, _, s1, _ = thrice(sim, "dots", n, vin, sin, variant=1)
        check_dot(s1[kr.S_D1], vin[X, :n], vin[R, :n], ("dots one", n))
        check_untouched(vin, v, sin, s1, n, scal_written=[kr.S_D1], what=("dots one", n))
        print("  n %-8d dot error / bar %.3g, %.3g" % (n, e, e2))


# ---- k_waxpy, k_scale_to -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", classes(BIG))
def test_waxpy_and_scale_to_with_the_drivers_aliasing(sim, sizes):
    for n in sizes:
        rng = np.random.default_rng(2000 + n)
        vin, sin = vectors(rng, n), scalars(rng)
        ref, M = kr.waxpy(ALPHA, vin[X, :n], vin[R, :n])
        outs = []
        for variant, dst in ((0, T), (1, X), (2, R)):   # w apart, w == x, w == y
            v, _, s, _ = thrice(sim, "waxpy", n, vin, sin, variant=variant, alpha=ALPHA)
            check_elem(v[dst, :n], ref, M, 8, ("waxpy", n, variant))
            check_untouched(vin, v, sin, s, n, vec_written=[dst], what=("waxpy", n, variant))
            outs.append(v[dst, :n])
        assert same(outs[0], outs[1]) and same(outs[0], outs[2]), ("aliasing changes the result", n)
        sin[kr.S_W2] = abs(sin[kr.S_W2])
        ref, M = kr.scale_to(vin[X, :n], sin[kr.S_W2])
        v0, _, s, _ = thrice(sim, "scale_to", n, vin, sin, variant=0)
        check_elem(v0[T, :n], ref, M, 8, ("scale_to", n))
        check_untouched(vin, v0, sin, s, n, vec_written=[T], what=("scale_to", n))
        v1, _, s, _ = thrice(sim, "scale_to", n, vin, sin, variant=1)   # in place
        assert same(v1[X, :n], v0[T, :n])
        check_untouched(vin, v1, sin, s, n, vec_written=[X], what=("scale_to in place", n))


# ---- the BiCGStab updates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", classes(BIG2))
def test_bcgs_updates_and_their_one_pass_form(sim, sizes, monkeypatch):
    for n in sizes:
        rng = np.random.default_rng(3000 + n)
        vin, sin = vectors(rng, n), scalars(rng)
        al, om, be = sin[kr.S_ALPHA], sin[kr.S_OMEGA], sin[kr.S_BETA]
        if n > 1023:   # (R,RP) of the updated R cancels to near zero
            vin[RP, :n] = cancelling(rng, vin[S, :n] - om * vin[T, :n])
        # P = R + beta (P - omega V)
        v, _, s, _ = thrice(sim, "bcgs_p", n, vin, sin)
        check_elem(v[P, :n], *kr.bcgs_p(vin[P, :n], vin[R, :n], vin[V, :n], be, om), 8, ("bcgs_p", n))
        check_untouched(vin, v, sin, s, n, vec_written=[P], what=("bcgs_p", n))
        # S = R - alpha V
        vs, _, s, _ = thrice(sim, "bcgs_s", n, vin, sin)
        check_elem(vs[S, :n], *kr.bcgs_s(vin[R, :n], vin[V, :n], al), 8, ("bcgs_s", n))
        check_untouched(vin, vs, sin, s, n, vec_written=[S], what=("bcgs_s", n))
        # X += alpha P + omega S, R = S - omega T: without the inner products, then with them finished four ways
        (xr, MX), (rr, MR) = kr.bcgs_xr(vin[X, :n], vin[P, :n], vin[S, :n], vin[T, :n], al, om)
        v0, _, s, _ = thrice(sim, "bcgs_xr", n, vin, sin, variant=0)
        check_elem(v0[X, :n], xr, MX, 8, ("bcgs_xr X", n))
        check_elem(v0[R, :n], rr, MR, 8, ("bcgs_xr R", n))
        check_untouched(vin, v0, sin, s, n, vec_written=[X, R], what=("bcgs_xr", n))
        sums = {}
        for tag, variant, env in (("launch", 1, False), ("k_finalize", 1, True), ("partials", 3, False), ("phase 4 + post", 2, False),
                                  ("phase 4 + post, k_finalize", 2, True)):
            if env:
                monkeypatch.setenv("WAI_FIN_SEPARATE", "1")
            v, _, s, post = thrice(sim, "bcgs_xr", n, vin, sin, variant=variant, times=3 if n <= 1023 or tag == "launch" else 1)
            monkeypatch.delenv("WAI_FIN_SEPARATE", raising=False)
            assert same(v, v0), ("the reduction changes the update", n, tag)
            if variant != 2:
                e1 = check_dot(s[kr.S_DP2], v[R, :n], v[R, :n], ("(R,R)", n, tag))
                e2 = check_dot(s[kr.S_RHONEW], v[R, :n], vin[RP, :n], ("(R,RP)", n, tag))
                check_untouched(vin, v, sin, s, n, vec_written=[X, R], scal_written=[kr.S_DP2, kr.S_RHONEW], what=("bcgs_xr", n, tag))
                assert np.isnan(post).all()
                sums[tag] = s
            else:
                own = sums["launch"]
                check_scalars(s, own, 4, ("bcgs_xr", n, tag))
                check_untouched(vin, v, sin, s, n, vec_written=[X, R], what=("bcgs_xr", n, tag),
                                scal_written=[kr.S_DP2, kr.S_RHONEW, kr.S_RHOOLD, kr.S_RHO, kr.S_BETA])
                assert same(post, [s[kr.S_DP2], s[kr.S_BREAK]]), ("post", n, tag, post, s[kr.S_DP2], s[kr.S_BREAK])
                sums[tag] = s
        # finished in the launch, by k_finalize and from the partial sums left behind: the same bits
        assert same(sums["launch"], sums["k_finalize"]) and same(sums["launch"], sums["partials"]), n
        assert same(sums["phase 4 + post"], sums["phase 4 + post, k_finalize"]), n
        print("  n %-8d (R,R) / bar %.3g  (R,RP) / bar %.3g" % (n, e1, e2))
        # the one-pass form: against the reference, and bit for bit against k_bcgs_s -> k_bcgs_xr<false> -> k_bcgs_p
        v1, _, s, _ = thrice(sim, "bcgs_xrp", n, vin, sin)
        (x1, MX), (r1, MR), (p1, MP) = kr.bcgs_xrp(vin[X, :n], vin[R, :n], vin[P, :n], vin[V, :n], vin[T, :n], al, om, be)
        check_elem(v1[X, :n], x1, MX, 8, ("bcgs_xrp X", n))
        check_elem(v1[R, :n], r1, MR, 8, ("bcgs_xrp R", n))
        check_elem(v1[P, :n], p1, MP, 8, ("bcgs_xrp P", n))
        check_untouched(vin, v1, sin, s, n, vec_written=[X, R, P], what=("bcgs_xrp", n))
        va, _, _, _ = sim.krylov_vec("bcgs_s", n, vin, sin)
        vb, _, _, _ = sim.krylov_vec("bcgs_xr", n, va, sin, variant=0)
        vc, _, _, _ = sim.krylov_vec("bcgs_p", n, vb, sin)
        for i, name in ((X, "X"), (R, "R"), (P, "P")):
            assert same(vc[i], v1[i]), ("k_bcgs_xrp against the three kernels it replaces", n, name)


def merged_scalars(rng, **kw):
    """scalars with five consistent merged sums: (T,T), (S,S) positive, Cauchy-Schwarz respected"""
    s = scalars(rng)
    s[kr.S_D2], s[kr.S_DP2] = abs(s[kr.S_D2]), abs(s[kr.S_DP2])
    s[kr.S_D1] = 0.6 * np.sqrt(s[kr.S_D2] * s[kr.S_DP2]) * np.sign(s[kr.S_D1])
    for name, v in kw.items():
        s[getattr(kr, "S_" + name)] = v
    return s


@pytest.mark.parametrize("sizes", classes(BIG2))
def test_bcgs_xrp_deriving_its_scalars(sim, sizes):
    """k_bcgs_xrp<true>: the scalars against the restated phase 6, the vectors against the reference with the launch's own
    omega and beta, and everything bit for bit against k_bcgs_scalars(6) followed by k_bcgs_xrp<false>"""
    for n in sizes:
        rng = np.random.default_rng(4000 + n)
        vin = vectors(rng, n)
        seeds = [("plain", merged_scalars(rng)),
                 ("code 3", merged_scalars(rng, D1=2.0, D2=4.0, RHONEW=3.0, W2=6.0)),      # rho = 3 - 0.5 * 6
                 ("code 2", merged_scalars(rng, D2=0.0))]                                  # omega = 0, beta = alpha / 0
        for tag, sin in seeds:
            v, _, s, post = thrice(sim, "bcgs_xrp_derive", n, vin, sin)
            check_scalars(s, sin, 6, ("bcgs_xrp_derive", n, tag))
            assert s[kr.S_BREAK] == {"plain": 0.0, "code 3": 3.0, "code 2": 2.0}[tag], (n, tag, s[kr.S_BREAK])
            assert tag != "code 2" or s[kr.S_OMEGA] == 0.0
            assert same(post, [s[kr.S_DP2], s[kr.S_BREAK]]), ("post", n, tag)
            written = [kr.S_OMEGA, kr.S_DP2, kr.S_RHONEW, kr.S_RHOOLD, kr.S_RHO, kr.S_BETA, kr.S_BREAK]
            check_untouched(vin, v, sin, s, n, vec_written=[X, R, P], scal_written=written, what=("bcgs_xrp_derive", n, tag))
            if tag != "code 2":   # (beta is infinite there: P is not a number the reference could be held to)
                (x1, MX), (r1, MR), (p1, MP) = kr.bcgs_xrp(vin[X, :n], vin[R, :n], vin[P, :n], vin[V, :n], vin[T, :n],
                                                           s[kr.S_ALPHA], s[kr.S_OMEGA], s[kr.S_BETA])
                check_elem(v[X, :n], x1, MX, 8, ("bcgs_xrp_derive X", n, tag))
                check_elem(v[R, :n], r1, MR, 8, ("bcgs_xrp_derive R", n, tag))
                check_elem(v[P, :n], p1, MP, 8, ("bcgs_xrp_derive P", n, tag))
            _, _, s6, post6 = sim.krylov_vec("scalars", n, vin, sin, variant=6)
            v6, _, s6b, _ = sim.krylov_vec("bcgs_xrp", n, vin, s6)
            assert same(s6, s6b)
            assert same(s, s6), ("k_bcgs_xrp<true> against k_bcgs_scalars(6): scalars", n, tag, s[:16], s6[:16])
            assert same(post, post6), ("post", n, tag)
            # (code 2: beta is infinite and P a NaN in both forms; a NaN's sign and payload are nobody's claim)
            assert same(v, v6) or (tag == "code 2" and np.array_equal(v, v6, equal_nan=True)), \
                ("k_bcgs_xrp<true> against k_bcgs_scalars(6) + k_bcgs_xrp<false>: vectors", n, tag)


def test_bcgs_xrp_derive_leaves_its_counter_at_zero(sim):
    """two k_bcgs_xrp<true> launches back to back in one context, the second at another n: a counter left above zero
    would let workgroup 0 of the second launch rotate the scalars before the others have read them (or report code 4)"""
    rng = np.random.default_rng(4999)
    for n in (262145, 3, 513, 1572867, 257):   # 1024 workgroups, 1, 3, 1024 again, 2
        vin, sin = vectors(rng, n), merged_scalars(rng)
        v, _, s, post = sim.krylov_vec("bcgs_xrp_derive", n, vin, sin)
        check_scalars(s, sin, 6, ("counter", n))
        assert s[kr.S_BREAK] == 0.0 and same(post, [s[kr.S_DP2], 0.0])
        _, _, s6, _ = sim.krylov_vec("scalars", n, vin, sin, variant=6)
        v6, _, _, _ = sim.krylov_vec("bcgs_xrp", n, vin, s6)
        assert same(s, s6) and same(v, v6), n


# ---- k_bcgs_scalars: every phase, every breakdown code --------------------------------------------------------------------
def test_derived_scalars_and_breakdown_codes(sim, monkeypatch):
    rng = np.random.default_rng(5000)
    vin = vectors(rng, 3)
    cases = []
    for phase in (0, 2, 3, 4, 5, 6):
        for _ in range(4):
            cases.append((phase, merged_scalars(rng), 0.0))
    cases += [(2, merged_scalars(rng, D1=0.0), 1.0),                                   # (V,RP) = 0
              (0, merged_scalars(rng, DP2=0.0), 1.0),                                  # rho = (R,R) = 0
              (3, merged_scalars(rng, D2=0.0), 2.0), (5, merged_scalars(rng, D2=0.0), 2.0), (6, merged_scalars(rng, D2=0.0), 2.0),
              (4, merged_scalars(rng, RHONEW=0.0), 3.0),                               # the next rho vanishes
              (6, merged_scalars(rng, D1=2.0, D2=4.0, RHONEW=3.0, W2=6.0), 3.0),
              (0, merged_scalars(rng, BREAK=4.0), 4.0),                                # a lost partial sum's code survives the start
              (0, merged_scalars(rng, BREAK=3.0), 0.0), (4, merged_scalars(rng, BREAK=2.0, RHONEW=0.0), 2.0)]
    for phase, sin, code in cases:
        v, _, s, post = thrice(sim, "scalars", 3, vin, sin, variant=phase)
        want = check_scalars(s, sin, phase, ("scalars", phase, code))
        assert s[kr.S_BREAK] == code == want[kr.S_BREAK], (phase, code, s[kr.S_BREAK], want[kr.S_BREAK])
        if code == 2.0 and phase != 4:   # (T,T) = 0 found by this phase
            assert s[kr.S_OMEGA] == 0.0
        _, scale = kr.derive(sin, phase)
        check_untouched(vin, v, sin, s, 3, scal_written=list(scale), what=("scalars", phase))
        if phase == 6:
            assert same(post, [s[kr.S_DP2], s[kr.S_BREAK]])
        else:
            assert np.isnan(post).all()
    # (R,RP) = 0 through k_bcgs_xr's own finaliser: code 3 from the launch's sum
    sin = scalars(rng)
    vin[RP, :] = 0.0
    for env in (False, True):
        if env:
            monkeypatch.setenv("WAI_FIN_SEPARATE", "1")
        _, _, s, post = sim.krylov_vec("bcgs_xr", 3, vin, sin, variant=2)
        monkeypatch.delenv("WAI_FIN_SEPARATE", raising=False)
        assert s[kr.S_RHONEW] == 0.0 and s[kr.S_BREAK] == 3.0 and post[1] == 3.0 and same(post[0], s[kr.S_DP2])


# ---- GMRES: k_mdot<1..8>, k_maxpy_norm, k_update_x -----------------------------------------------------------------------
def basis_sets(sizes, seed):
    """per n: (n, basis counts, vectors, scalars, basis vectors (largest count, n)) -- a case takes the first k of them, so
    one long-double reference per n serves every k and leading dimension.  In the big cases the first basis vector is
    T's cancelling partner"""
    for n in sizes:
        rng = np.random.default_rng(seed + n)
        ks = K_SMALL if n <= 1023 else K_BIG
        vin, sin = vectors(rng, n), scalars(rng)
        B = rng.normal(size=(max(ks), n))
        if n > 1023:
            B[0] = cancelling(rng, vin[T, :n])
        yield n, ks, vin, sin, B


def layouts(B, n, k):
    """(ld, the first k basis vectors ld apart with guards between and a guard vector behind) for ld = n, n + 1, n + 16"""
    for pad in (0, 1, 16):
        packed = np.full((k + 1, n + pad), SENT)
        packed[:k, :n] = B[:k]
        yield n + pad, packed.ravel()


def repeats(n, ldim):
    return 3 if ldim == n + 1 else 1


@pytest.mark.parametrize("sizes", classes(BIG2))
def test_mdot_every_count_and_leading_dimension(sim, sizes):
    worst = 0.0
    for n, ks, vin, sin, B in basis_sets(sizes, 6000):
        d, bar = kr.mdot(vin[T], B.ravel(), n, len(B), n)
        for k in ks:
            for ldim, bin_ in layouts(B, n, k):
                v, b, s, _ = thrice(sim, "mdot", n, vin, sin, k=k, ld=ldim, basis=bin_, times=repeats(n, ldim))
                for j in range(k):
                    err = float(abs(LD(s[kr.S_H + j]) - d[j]) / (LD(1e-13) * bar[j]))
                    worst = max(worst, err)
                    assert err <= 1.0, ("mdot", n, k, ldim, j, s[kr.S_H + j], float(d[j]), err)
                check_untouched(vin, v, sin, s, n, scal_written=range(kr.S_H, kr.S_H + k), what=("mdot", n, k, ldim))
                check_basis_untouched(bin_, b, ("mdot", n, k, ldim))
    WORST["dot"] = max(WORST["dot"], worst)
    print("  mdot: largest error / bar %.3g" % worst)


def partial_updates(v0, B, coef, sign):
    """v0 + sign * sum_{j < k} coef_j v_j and its magnitude sum for every k at once (index k - 1), in long double"""
    t = ld_(coef)[:len(B), None] * ld_(B)
    return ld_(v0)[None, :] + LD(sign) * np.cumsum(t, axis=0), np.abs(ld_(v0))[None, :] + np.cumsum(np.abs(t), axis=0)


@pytest.mark.parametrize("sizes", classes(BIG2))
def test_maxpy_norm_update_and_its_norm(sim, sizes):
    worst_e, worst_d = 0.0, 0.0
    for n, ks, vin, sin, B in basis_sets(sizes, 7000):
        refs, Ms = partial_updates(vin[T, :n], B, sin[kr.S_H:kr.S_H + len(B)], -1)
        for k in ks:
            for ldim, bin_ in layouts(B, n, k):
                v, b, s, _ = thrice(sim, "maxpy_norm", n, vin, sin, k=k, ld=ldim, basis=bin_, times=repeats(n, ldim))
                err = np.abs(ld_(v[T, :n]) - refs[k - 1]) / (LD(2 * (k + 2)) * LD(kr.U) * Ms[k - 1])
                worst_e = max(worst_e, float(err.max()))
                assert err.max() <= 1.0, ("maxpy_norm w", n, k, ldim, int(np.argmax(err)), float(err.max()))
                # the reduction alone: |w|^2 of the w the launch returned
                worst_d = max(worst_d, check_dot(s[kr.S_W2], v[T, :n], v[T, :n], ("maxpy_norm |w|^2", n, k, ldim)))
                check_untouched(vin, v, sin, s, n, vec_written=[T], scal_written=[kr.S_W2], what=("maxpy_norm", n, k, ldim))
                check_basis_untouched(bin_, b, ("maxpy_norm", n, k, ldim))
    WORST["elem"] = max(WORST["elem"], worst_e)
    print("  maxpy_norm: largest element error / bar %.3g, |w|^2 error / bar %.3g" % (worst_e, worst_d))


@pytest.mark.parametrize("sizes", classes(BIG))
def test_update_x(sim, sizes):
    worst = 0.0
    for n, ks, vin, sin, B in basis_sets(sizes, 8000):
        coef = signed(np.random.default_rng(8500 + n), len(B))
        refs, Ms = partial_updates(vin[X, :n], B, coef, 1)
        for k in ks:
            for ldim, bin_ in layouts(B, n, k):
                v, b, s, _ = thrice(sim, "update_x", n, vin, sin, k=k, ld=ldim, basis=bin_, coef=coef[:k], times=repeats(n, ldim))
                err = np.abs(ld_(v[X, :n]) - refs[k - 1]) / (LD(2 * (k + 2)) * LD(kr.U) * Ms[k - 1])
                worst = max(worst, float(err.max()))
                assert err.max() <= 1.0, ("update_x", n, k, ldim, int(np.argmax(err)), float(err.max()))
                assert same(s[kr.COEF:kr.COEF + k], coef[:k])          # the coefficients travel through the scalars' tail
                check_untouched(vin, v, sin, s, n, vec_written=[X], scal_written=range(kr.COEF, kr.COEF + k), what=("update_x", n, k, ldim))
                check_basis_untouched(bin_, b, ("update_x", n, k, ldim))
    WORST["elem"] = max(WORST["elem"], worst)
    print("  update_x: largest element error / bar %.3g" % worst)


# ---- the entry point itself ----------------------------------------------------------------------------------------------
def test_refusals_and_temporaries(sim):
    rng = np.random.default_rng(9000)
    vin, sin = vectors(rng, 8), scalars(rng)
    basis = make_basis(rng, 8, 9, 2)
    sim.krylov_vec("mdot", 8, vin, sin, k=2, ld=9, basis=basis)      # (whatever the first call sets up lazily is set up)
    before = device_memory()
    sim.krylov_vec("mdot", 8, vin, sin, k=2, ld=9, basis=basis)
    sim.krylov_vec("bcgs_xrp_derive", 8, vin, sin)
    assert device_memory() == before                                  # the temporaries are returned before the call ends
    launches = sim.launch_stats()[0]
    for kw, why in ((dict(op="dot", n=0), "n < 1"), (dict(op="dot", n=14), "len < n"), (dict(op="mdot", n=8, k=0, ld=9, basis=np.zeros(9)), "basis count"),
                    (dict(op="mdot", n=8, k=41, ld=9, basis=np.zeros(42 * 9)), "basis count"),
                    (dict(op="mdot", n=8, k=2, ld=7, basis=np.zeros(21)), "ld < n"), (dict(op="waxpy", n=8, variant=3), "variant")):
        op, n = kw.pop("op"), kw.pop("n")
        with pytest.raises(WaiError, match=r"\(-2\).*" + why):
            sim.krylov_vec(op, n, vin, sin, **kw)
    assert sim.launch_stats()[0] == launches and device_memory() == before   # refused before anything is launched


# ---- GMRES end to end: the residual estimate must be honest -----------------------------------------------------------------
def test_gmres_estimate_is_honest(oracle):
    """GMRES on the 12 x 10 x 9 eos-we system of test_hip_parity.py::test_spmv_ilu_krylov at rtol 1e-10: the norm the solver
    returns (the Givens recurrence's estimate) against the true preconditioned residual |B^-1 (b - A x)| formed with
    spmv and pc_apply, as a fraction of |B^-1 b|.  Classical Gram-Schmidt with a wrong coefficient loses orthogonality
    and the estimate drifts from the truth long before the solve stops converging; the oracle's GMRES on the same system
    gives the gap a correct one has, and the device's must stay within 10 x that (another summation order).

    The solve needs 135 iterations and the basis holds at most 40 vectors (MAX_RESTART), so a single cycle cannot reach
    1e-10 here.  Two runs instead: the whole solve at restart 40 (four cycles; the iteration counts must be EQUAL), and one
    cycle of 40 iterations alone (ksp_max_its 40: no restart refreshes the residual, the estimate is the recurrence's
    throughout, both stop at 40).

    The gap cannot be resolved below one rounding of the scale it is measured on: b - A x is a difference of entries of
    the size of b, each rounded to 2^-53 of that, so |B^-1 (b - A x)| is known to about 2^-53 |B^-1 b| and a gap below that
    is chance.  The oracle's gap is such a figure: its inner products are OpenMP reductions, and with another team size
    the same solve gave 3.9e-16 and 1.6e-17.  So the reference gap is the oracle's, but not less than 2^-53.
    MEASURED (MI355X): whole solve 135 = 135 iterations, gap 2.6e-16 (estimate 1.268421e-09 against a true 1.268418e-09);
    oracle 3.9e-16 in one run of this file, 1.6e-17 in a run of the whole suite.  One cycle: 40 = 40 iterations at
    5.482967e-03, gap 1.0e-18 (oracle 6.1e-16)."""
    from oracle import binding as ol
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(12, 10, 9), brick=(4, 4, 4), eos="we")
    sim = FlowSimulation(lm, eos="we")
    osim = ol.OracleSim(oracle, lm, 1)
    sim.set_regions(region); osim.set_regions(region)
    yo = osim.yvec(scaled(prim, region, "we").ravel().copy())
    assert osim.pre_eval(yo) == 0
    L = osim.lhs()
    err, b = osim.residual(yo, 5.0e4, L)
    err, J = osim.jacobian(yo, 5.0e4, L, b, mode=0)
    assert err == 0
    sim.set_jacobian_values(J)
    rp, ci = osim.pattern()
    n = sim.num_dof
    for tag, maxits, reasons in (("whole solve", 10000, (2, 2)), ("one cycle", 40, (-3, -3))):
        sim.set_opts(ksp_type="gmres", gmres_restart=40, ksp_rtol=1e-10, ksp_max_its=maxits)
        x = np.zeros(n)
        its, reason, est = sim.ksp_solve(b, x)
        oreason, xo, oits, hist = osim.ksp_solve(J, b, ksp_type=1, restart=40, rtol=1e-10, maxits=maxits)
        assert (reason, oreason) == reasons, (tag, reason, oreason)
        # the device's truth, with its own operator and preconditioner
        ax, z = np.zeros(n), np.zeros(n)
        assert sim.spmv(x, ax) == 0 and sim.pc_apply(b - ax, z) == 0
        true = float(np.linalg.norm(z))
        # the oracle's, with the oracle's
        axo = np.zeros(n)
        oracle.wo_bcsr_spmv(sim.n_owned, 2, ol.ip(rp), ol.ip(ci), ol.dp(J), ol.dp(osim.yvec(xo)), ol.dp(axo))
        osim.pc_setup(J)
        otrue = float(np.linalg.norm(osim.pc_apply(b - axo)))
        gap, ogap = abs(est - true) / hist[0], abs(hist[-1] - otrue) / hist[0]
        print("  %-12s its %d (oracle %d)  estimate %.6e true %.6e gap %.3g  oracle: estimate %.6e true %.6e gap %.3g"
              % (tag, its, oits, est, true, gap, hist[-1], otrue, ogap))
        assert its == oits, (tag, its, oits)
        assert gap <= 10.0 * max(ogap, 2.0 ** -53), (tag, gap, ogap)
    sim.destroy(); osim.close()
