"""The source network's pass on the device (wai_set_network_pass, k_network_pass) and the coupling build without host waits:
the host pass (the same network_pass, run on the host) must give the same bits -- one pass (wai_test_network_pass against
wai_network_evaluate, which tests/test_network_pass_host.py holds to the recorded bits of the former recursion), a residual, the
rates, the network's state and coupling blocks, a Newton step and whole input runs, host mode against device mode -- and the
stream waits the passes and the coupling build issue are counted in both modes."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import network_cases as nc
from tests import test_hip_memory as tm
from waiwera_amd import lib as wl
from waiwera_amd.cases import make_case, scaled

pytestmark = pytest.mark.gpu
INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
GUARD = -4.25e77


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def P(a):
    return a.ctypes.data_as(wl.pi if a.dtype == np.int32 else wl.pd)


class DeviceVector:
    """a vector in device memory from the HIP runtime the library itself runs on: what the library does to a vector it is
    handed IN PLACE (wai_jacobian perturbs and restores y) shows only there -- a host array is staged"""
    hip = None

    def __init__(self, a):
        if DeviceVector.hip is None:
            # the copy of the runtime this process has mapped -- the one the library is bound to (wl is imported): a second
            # copy loaded from elsewhere would not share its device context
            path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line)
            DeviceVector.hip = C.CDLL(path)
            DeviceVector.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            DeviceVector.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            DeviceVector.hip.hipFree.argtypes = [C.c_void_p]
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.n, p = a.size, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), a.nbytes) == 0
        self.p = p.value
        assert self.hip.hipMemcpy(self.p, a.ctypes.data, a.nbytes, 1) == 0      # host to device

    def __int__(self):      # lib.ptr takes it as a raw address
        return self.p

    def host(self):
        out = np.zeros(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data, self.p, out.nbytes, 2) == 0  # device to host (waits for the device)
        return out

    def free(self):
        self.hip.hipFree(self.p)


@pytest.fixture(scope="module")
def small():
    """a 4 x 4 x 2 `we` mesh; the tests put their own sources on it"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(4, 4, 2), brick=(2, 2, 2), eos="we", sources=False)
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    yield sim, lm
    sim.destroy()


def carry(sim, lm, c):
    """the case's sources (their own rates and enthalpies, separators as control records) and network on the context"""
    n = len(c["rate"])
    cell = wl._i32(np.arange(n) % lm.n_owned)
    rate, enth, comp = wl._f64(c["rate"]), wl._f64(c["enth"]), wl._i32(np.zeros(n))
    sim._chk(wl.LIB.wai_set_sources(sim.h, n, P(cell), P(rate), P(enth), P(comp)), "set_sources")
    recs = []
    for i in range(n):
        s = c["sep"][8 * i: 8 * i + 8]
        recs.append(dict(sep_hf=s[0], sep_hg=s[1], sep_more=[(s[2 + 2 * q], s[3 + 2 * q]) for q in range(3)]))
    sim._chk(wl.LIB.wai_set_source_controls(sim.h, wl.source_controls(recs)), "set_source_controls")
    sim.set_source_network(c["spec"])


def device_pass(sim, c):
    """(sources, groups, reinjectors, net, enth) of one k_network_pass, each array checked for a guard behind it"""
    n, ng, nr = len(c["rate"]), len(c["spec"]["groups"]), len(c["spec"]["reinjectors"])
    raw = wl._f64(np.concatenate([c["rate"], c["enth"]]))
    out = [np.full(k + 1, GUARD) for k in (6 * n, 6 * ng, 8 * nr, 2 * n, n)]
    sim._chk(wl.LIB.wai_test_network_pass(sim.h, P(raw), *[P(a) for a in out]), "test_network_pass")
    for a in out:
        assert a[-1] == GUARD
    return [a[:-1] for a in out]


def check_pass(sim, lm, c):
    carry(sim, lm, c)
    S, G, R = wl.network_evaluate(c["spec"], c["rate"], c["enth"], c["sep"])
    s, g, r, net, enth = device_pass(sim, c)
    assert same_bits(s, S), np.argwhere(s.reshape(S.shape) != S)
    assert same_bits(g, G) and same_bits(r, R)
    want_net, fed, fed_enth = nc.handed_over(c, S)
    assert same_bits(net, want_net)
    want = c["enth"].copy()      # what wai_set_sources put there: untouched for the sources nobody feeds
    want[fed] = fed_enth
    assert same_bits(enth, want)
    return fed


def fixture_case(oracle):
    from oracle import binding as ol
    e = ol.Eos()
    oracle.wo_eos_init(C.byref(e), 1)

    def sep_enth(p):
        hf, hg = np.zeros(1), np.zeros(1)
        assert oracle.wo_separator_enthalpies(C.byref(e), float(p), ol.dp(hf), ol.dp(hg)) == 0
        return float(hf[0]), float(hg[0])
    return nc.reference_fixture(sep_enth)


# ---- 1. one pass against the host's ------------------------------------------------------------------------------------------
def test_pass_reference_fixture(small, oracle):
    sim, lm = small
    c = fixture_case(oracle)
    fed = check_pass(sim, lm, c)
    assert len(fed) > 0 and len(fed) < len(c["rate"])


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_pass_source_counts_at_the_lanes_edges(small, oracle, n):
    """the fixture's network with further producers behind a limit of their own: 63, 64, 65 and 130 sources in all"""
    sim, lm = small
    check_pass(sim, lm, nc.with_sources(fixture_case(oracle), n))


@pytest.mark.parametrize("name", ["uniform", "progressive", "nested", "nested_deep_cut", "water_uniform", "water_progressive",
                                  "steam_uniform", "steam_progressive", "chain", "chain_short", "zero", "positive"])
def test_pass_limiters_nesting_and_chains(small, name):
    sim, lm = small
    c = dict(uniform=lambda: nc.three_wells(0), progressive=lambda: nc.three_wells(1), nested=nc.nested,
             nested_deep_cut=lambda: nc.nested(3.0), water_uniform=lambda: nc.separated_limit(1, 0),
             water_progressive=lambda: nc.separated_limit(1, 1), steam_uniform=lambda: nc.separated_limit(2, 0),
             steam_progressive=lambda: nc.separated_limit(2, 1), chain=nc.chain,
             chain_short=lambda: nc.chain((-6.0, -4.0, 0.0, 0.2, 0.0, 0.0)), zero=lambda: nc.signs()[0],
             positive=lambda: nc.signs()[1])[name]()
    check_pass(sim, lm, c)


# ---- 2., 3. host mode against device mode -----------------------------------------------------------------------------------
def coupled_pair():
    """two contexts on one state: producers on deliverability behind a limited group whose water feeds two injectors through
    a reinjector, the rest overflowing to a third (the arrangement of test_source_network_across_ranks, on one rank)"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=tm.DIMS, brick=tm.BRICK, eos="we", lens=True)
    controls, spec = tm.network(lm)
    rate = np.asarray(lm.src_rate)
    inj = [int(i) for i in np.flatnonzero(rate > 0)]
    spec["reinjectors"][0]["overflow"] = (1, inj[1])
    y = scaled(prim, region, "we").ravel().copy()
    sims = {}
    for where in ("host", "device"):
        sim = FlowSimulation(lm, eos="we")
        sim.set_regions(region)
        if where == "device":
            sim.set_network_pass("device")      # before the network is set ...
        sim.set_source_controls(controls)
        sim.set_source_network(spec)
        assert sim.network_pass() == (where, where)
        sims[where] = sim
    return lm, y, sims


def test_host_and_device_modes_agree_bit_for_bit():
    lm, y, sims = coupled_pair()
    got = {}
    for where, sim in sims.items():
        n = sim.num_dof
        L, f = np.zeros(n), np.zeros(n)
        assert sim.pre_eval(0.0, y) == 0
        sim.lhs(0.0, (0.0, 0.0), y, L)
        assert sim.residual(0.0, tm.DT, y, L, f) == 0
        rates = sim.source_rates()
        G, R = sim.source_network()
        sep = sim.source_separated()
        yd, Ld = DeviceVector(y), DeviceVector(L)
        assert sim.jacobian(0.0, tm.DT, yd, Ld) == 0
        sim.synchronize()
        assert same_bits(yd.host(), y), "y after wai_jacobian is y before it"
        yd.free(); Ld.free()
        cells, E = sim.network_couplings()
        y1, f1 = y.copy(), np.zeros(n)
        reason, kits, rnorm = sim.newton_step(0.0, tm.DT, 0, y1, L, f1)
        got[where] = dict(f=f, rate=rates[0], enth=rates[1], G=G, R=R, sep=sep, cells=cells, E=E, y1=y1, f1=f1, kits=kits, reason=reason)
        sim.destroy()
    h, d = got["host"], got["device"]
    assert len(h["cells"]) == 7 and np.abs(h["E"]).max() > 0 and h["reason"] > 0    # four producers, three fed injectors
    assert abs(h["rate"][h["rate"] < 0].sum() + 12.0) < 1e-9                      # the limiter is at work
    assert np.array_equal(h["cells"], d["cells"]) and (h["kits"], h["reason"]) == (d["kits"], d["reason"])
    for key in ("f", "rate", "enth", "G", "R", "sep", "E", "y1", "f1"):
        assert same_bits(h[key], d[key]), key


def test_stream_waits_are_gone_in_device_mode():
    lm, y, sims = coupled_pair()
    grew = {}
    for where, sim in sims.items():
        n = sim.num_dof
        L, f = np.zeros(n), np.zeros(n)
        assert sim.pre_eval(0.0, y) == 0
        sim.lhs(0.0, (0.0, 0.0), y, L)
        assert sim.residual(0.0, tm.DT, y, L, f) == 0      # (the first device pass uploads the description: one wait, once)
        p0, w0 = sim.network_stats()
        assert sim.residual(0.0, tm.DT, y, L, f) == 0
        p1, w1 = sim.network_stats()
        assert sim.jacobian(0.0, tm.DT, y, L) == 0
        p2, w2 = sim.network_stats()
        m = len(sim.network_couplings()[0])
        grew[where] = (p1 - p0, w1 - w0, p2 - p1, w2 - w1, m)
        sim.destroy()
    bs = 2
    hp, hw, hjp, hjw, m = grew["host"]
    dp, dw, djp, djw, dm = grew["device"]
    assert m == dm == 7
    assert (hp, hjp) == (dp, djp) and hp >= 1 and hjp >= 2 * m * bs       # the same passes either way: two per column and more
    assert hw >= 2 and hjw >= 2 * m * bs
    assert dw == 0 and djw <= 1


# ---- 4. whole input runs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,geometry", [("reinjection", "greinjection.dat"), ("makeup_progressive", "gmakeup.dat")])
def test_input_runs_identical_in_device_mode(name, geometry):
    from waiwera_amd.simulation import Simulation
    runs = {}
    for where in ("host", "device"):
        kw = {} if where == "host" else dict(network_pass="device")
        sim = Simulation.from_json(os.path.join(INPUTS, name + ".json"), mesh_file=os.path.join(INPUTS, geometry), **kw)
        assert sim.network_pass_choice == (where, where)
        out = sim.run()
        runs[where] = (list(sim.ts.history), out, sim.ode.network_stats())
        sim.ode.destroy()
    (hh, ho, hs), (dh, do, ds) = runs["host"], runs["device"]
    assert len(hh) > 0 and [tuple(x) for x in hh] == [tuple(x) for x in dh]
    assert sorted(ho) == sorted(do)
    for key in ho:
        a, b = np.asarray(ho[key]), np.asarray(do[key])
        assert (same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)), key
    assert hs[0] == ds[0] > 0 and ds[1] < hs[1]


# ---- 5. fall-backs ------------------------------------------------------------------------------------------------------
def test_network_too_large_for_lds_keeps_the_host_pass(small):
    """sources in one flat group until description and state pass the builder's limit: asked for the device, the host pass
    stays in force and gives the host pass' results"""
    sim, lm = small
    limit, needed = C.c_int(0), C.c_int(0)

    def flat(n):
        spec = dict(rate_specified=[1] * n, enthalpy_specified=[0] * n, reinjectors=[],
                    groups=[dict(inputs=[(1, i) for i in range(n)], scaling=0, limits=[(0, 0.3 * n)], separator=None)])
        k = np.arange(n)
        return nc.case(spec, -0.5 - 0.01 * (k % 7), 1.0e6 + 1.0e3 * k, nc.separators(n, range(0, n, 3)))
    sim.set_network_pass("device")
    try:
        carry(sim, lm, flat(64))
        sim._chk(wl.LIB.wai_test_network_lds(sim.h, C.byref(limit), C.byref(needed)), "network_lds")
        assert limit.value == 8192 and 0 < needed.value <= limit.value and sim.network_pass() == ("device", "device")
        per_source = needed.value / 64.0
        n = int(limit.value / per_source) + 16      # past the limit by the builder's own count
        c = flat(n)
        carry(sim, lm, c)
        sim._chk(wl.LIB.wai_test_network_lds(sim.h, C.byref(limit), C.byref(needed)), "network_lds")
        assert needed.value > limit.value and sim.network_pass() == ("device", "host")
        with pytest.raises(wl.WaiError):
            device_pass(sim, c)
        g, lm2, prim, region = make_case(dims=(4, 4, 2), brick=(2, 2, 2), eos="we", sources=False)
        y = scaled(prim, region, "we").ravel().copy()
        assert sim.pre_eval(0.0, y) == 0
        p0, w0 = sim.network_stats()
        rate = np.zeros(n)
        sim._chk(wl.LIB.wai_get_source_rates(sim.h, P(rate), None), "get_source_rates")
        p1, w1 = sim.network_stats()
        assert p1 - p0 == 1 and w1 - w0 >= 2                  # the host pass ran
        G, R = sim.source_network()
        assert abs(G[0, 0] + 0.3 * n) < 1e-9                  # ... and limited the group
        # the results are host mode's: the same calls with the host pass asked for
        sim.set_network_pass("host")
        assert sim.network_pass() == ("host", "host")
        rate_h = np.zeros(n)
        sim._chk(wl.LIB.wai_get_source_rates(sim.h, P(rate_h), None), "get_source_rates")
        G_h, R_h = sim.source_network()
        assert same_bits(rate, rate_h) and same_bits(G, G_h) and rate.min() < 0
    finally:
        sim.set_network_pass("host")


def test_unknown_place_is_refused(small):
    sim, lm = small
    with pytest.raises(wl.WaiError) as e:
        sim._chk(wl.LIB.wai_set_network_pass(sim.h, 2), "set_network_pass")
    assert "(-2)" in str(e.value) and "WAI_NETWORK_PASS_DEVICE" in str(e.value)
    with pytest.raises(ValueError):
        sim.set_network_pass("elsewhere")
    assert sim.network_pass()[0] == "host"
