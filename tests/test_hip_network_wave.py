"""The source network's device pass with the wave-wide walk (wai_set_network_walk, WAI_NETWORK_WALK_WAVE: k_network_pass_wave,
k_cb_pass_wave).  The host pass (the lane walk's network_pass, run on the host; tests/test_network_wave_host.py holds both
walks to the recorded bits of the former recursion) must give the same bits: one pass through wai_test_network_pass against
wai_network_evaluate with guard elements behind every output; a residual, the rates, the node states, the coupling blocks of
the column loop and of the batched build, a Newton step and whole input runs with walk=wave against walk=lane and host mode.
A network that needs more than the lane walk's 64 KB runs its pass on the device under the wave walk alone; one above 160 KiB
and one whose topology the wave schedule refuses keep what ran before.  Every case is a handful of one-wave launches on the
4 x 4 x 2 `we` mesh of tests/test_hip_network_device.py, whose helpers are used as they are."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import network_cases as nc
from tests import network_wave_cases as wc
from tests import test_hip_memory as tm
from tests.test_hip_network_device import INPUTS, DeviceVector, P, carry, check_pass, device_pass, fixture_case, same_bits
from waiwera_amd import lib as wl
from waiwera_amd.cases import make_case, scaled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wave():
    """a 4 x 4 x 2 `we` mesh with the device pass and the wave walk asked for; the tests put their own sources on it"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(4, 4, 2), brick=(2, 2, 2), eos="we", sources=False)
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    assert sim.network_walk() == ("lane", "lane")      # the default
    sim.set_network_pass("device")
    sim.set_network_walk("wave")      # before the network is set ...
    yield sim, lm
    sim.destroy()


def lds(sim):
    limit, needed = C.c_int(0), C.c_int(0)
    sim._chk(wl.LIB.wai_test_network_lds(sim.h, C.byref(limit), C.byref(needed)), "network_lds")
    return limit.value, needed.value


def check_wave_pass(sim, lm, c):
    fed = check_pass(sim, lm, c)
    assert sim.network_walk() == ("wave", "wave") and sim.network_pass() == ("device", "device")
    assert lds(sim) == (wc.WAVE_LDS_DOUBLES, int(wc.schedule(c["spec"])["lds"][0]))
    return fed


# ---- 1. one pass against the host's ------------------------------------------------------------------------------------------
def test_pass_reference_fixture(wave, oracle):
    sim, lm = wave
    c = fixture_case(oracle)
    fed = check_wave_pass(sim, lm, c)
    assert 0 < len(fed) < len(c["rate"])


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_pass_source_counts_at_the_lanes_edges(wave, oracle, n):
    sim, lm = wave
    check_wave_pass(sim, lm, nc.with_sources(fixture_case(oracle), n))


@pytest.mark.parametrize("name", ["uniform", "progressive", "nested", "nested_deep_cut", "nested_idle", "water_uniform",
                                  "water_progressive", "steam_uniform", "steam_progressive", "chain", "chain_short", "chain_dry",
                                  "zero", "positive", "mixed", "negative_zero"])
def test_pass_limiters_nesting_and_chains(wave, name):
    sim, lm = wave
    c = dict(uniform=lambda: nc.three_wells(0), progressive=lambda: nc.three_wells(1), nested=nc.nested,
             nested_deep_cut=lambda: nc.nested(3.0), nested_idle=lambda: nc.nested(100.0), water_uniform=lambda: nc.separated_limit(1, 0),
             water_progressive=lambda: nc.separated_limit(1, 1), steam_uniform=lambda: nc.separated_limit(2, 0),
             steam_progressive=lambda: nc.separated_limit(2, 1), chain=nc.chain,
             chain_short=lambda: nc.chain((-6.0, -4.0, 0.0, 0.2, 0.0, 0.0)), chain_dry=lambda: nc.chain((0.0, 0.0, 0.0, 1.5, 0.0, 0.0)),
             zero=lambda: nc.signs()[0], positive=lambda: nc.signs()[1], mixed=lambda: nc.signs()[2],
             negative_zero=lambda: nc.signs()[3])[name]()
    check_wave_pass(sim, lm, c)


@pytest.mark.parametrize("scaling", [0, 1])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
def test_pass_wide_groups(wave, m, scaling):
    sim, lm = wave
    check_wave_pass(sim, lm, wc.wide_group(m, scaling))


@pytest.mark.parametrize("name", ["nested_wide", "nested_wide_cut", "reinjector_65", "two_outputs_one_source", "wide_random_3",
                                  "wide_random_11"])
def test_pass_wide_cases(wave, name):
    sim, lm = wave
    c = dict(nested_wide=wc.nested_wide, nested_wide_cut=lambda: wc.nested_wide(70, 6.0), reinjector_65=wc.wide_reinjector,
             two_outputs_one_source=wc.two_outputs_one_source, wide_random_3=lambda: wc.wide_random(3),
             wide_random_11=lambda: wc.wide_random(11))[name]()
    check_wave_pass(sim, lm, c)


# ---- 2. host mode, the lane walk and the wave walk on one state ----------------------------------------------------------------
MODES = [("host", "lane", "columns"), ("device", "lane", "columns"), ("device", "wave", "columns"), ("device", "lane", "batched"),
         ("device", "wave", "batched")]


def test_modes_agree_bit_for_bit():
    """producers on deliverability behind a limited group whose water feeds two injectors through a reinjector, the rest
    overflowing to a third (the arrangement of tests/test_hip_network_device.py): residual, rates, node states, coupling blocks
    and one Newton step"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=tm.DIMS, brick=tm.BRICK, eos="we", lens=True)
    controls, spec = tm.network(lm)
    inj = [int(i) for i in np.flatnonzero(np.asarray(lm.src_rate) > 0)]
    spec["reinjectors"][0]["overflow"] = (1, inj[1])
    y = scaled(prim, region, "we").ravel().copy()
    got = {}
    for where, walk, build in MODES:
        sim = FlowSimulation(lm, eos="we")
        sim.set_regions(region)
        sim.set_source_controls(controls)
        sim.set_source_network(spec)
        sim.set_network_pass(where)      # ... and after it
        sim.set_network_walk(walk)
        sim.set_coupling_build(build)
        assert sim.network_pass() == (where, where) and sim.coupling_build() == (build, build)
        assert sim.network_walk() == (walk, walk)
        n = sim.num_dof
        L, f = np.zeros(n), np.zeros(n)
        assert sim.pre_eval(0.0, y) == 0
        sim.lhs(0.0, (0.0, 0.0), y, L)
        assert sim.residual(0.0, tm.DT, y, L, f) == 0
        p0, w0 = sim.network_stats()
        assert sim.residual(0.0, tm.DT, y, L, f) == 0
        p1, w1 = sim.network_stats()
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
        got[(where, walk, build)] = dict(f=f, rate=rates[0], enth=rates[1], G=G, R=R, sep=sep, cells=cells, E=E, y1=y1, f1=f1,
                                         kits=kits, reason=reason, waits=w1 - w0, passes=p1 - p0)
        sim.destroy()
    h = got[MODES[0]]
    assert len(h["cells"]) == 7 and np.abs(h["E"]).max() > 0 and h["reason"] > 0
    assert abs(h["rate"][h["rate"] < 0].sum() + 12.0) < 1e-9      # the limiter is at work
    for mode in MODES[1:]:
        d = got[mode]
        assert np.array_equal(h["cells"], d["cells"]) and (h["kits"], h["reason"]) == (d["kits"], d["reason"]), mode
        for key in ("f", "rate", "enth", "G", "R", "sep", "E", "y1", "f1"):
            assert same_bits(h[key], d[key]), (mode, key)
        assert d["waits"] == 0 and d["passes"] == h["passes"], mode
    assert h["waits"] >= 2


# ---- 3. whole input runs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,geometry", [("reinjection", "greinjection.dat"), ("makeup_progressive", "gmakeup.dat")])
def test_input_runs_identical_under_the_wave_walk(name, geometry):
    from waiwera_amd.simulation import Simulation
    runs = {}
    for mode in ("host", "lane", "wave"):
        kw = {} if mode == "host" else dict(network_pass="device", network_walk=mode)
        sim = Simulation.from_json(os.path.join(INPUTS, name + ".json"), mesh_file=os.path.join(INPUTS, geometry), **kw)
        assert sim.network_pass_choice == (("host", "host") if mode == "host" else ("device", "device"))
        assert sim.network_walk_choice == (("wave", "wave") if mode == "wave" else ("lane", "lane"))
        out = sim.run()
        runs[mode] = (list(sim.ts.history), out, sim.ode.network_stats())
        sim.ode.destroy()
    hh, ho, hs = runs["host"]
    for mode in ("lane", "wave"):
        dh, do, ds = runs[mode]
        assert len(hh) > 0 and [tuple(x) for x in hh] == [tuple(x) for x in dh], mode
        assert sorted(ho) == sorted(do)
        for key in ho:
            a, b = np.asarray(ho[key]), np.asarray(do[key])
            assert (same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)), (mode, key)
        assert hs[0] == ds[0] > 0 and ds[1] < hs[1], mode


# ---- 4. what only the wave walk holds on the device, and what it leaves alone ------------------------------------------------
def small_state():
    g, lm2, prim, region = make_case(dims=(4, 4, 2), brick=(2, 2, 2), eos="we", sources=False)
    return scaled(prim, region, "we").ravel().copy()


def test_network_between_64_kb_and_160_kib_runs_on_the_device_under_the_wave_walk(wave):
    """450 flat producers behind one limit and a reinjector: more than 8192 doubles, fewer than 20480"""
    sim, lm = wave
    c = wc.flat_behind_limit(450)
    n = len(c["rate"])
    sch = wc.schedule(c["spec"])
    assert 8192 < sch["lane_lds"] and sch["lds"][0] < wc.WAVE_LDS_DOUBLES
    try:
        sim.set_network_walk("lane")
        carry(sim, lm, c)
        assert lds(sim) == (8192, sch["lane_lds"])
        assert sim.network_pass() == ("device", "host") and sim.network_walk() == ("lane", "lane")      # as before
        with pytest.raises(wl.WaiError):
            device_pass(sim, c)
        y = small_state()
        assert sim.pre_eval(0.0, y) == 0
        rate_lane = np.zeros(n)
        p0, w0 = sim.network_stats()
        sim._chk(wl.LIB.wai_get_source_rates(sim.h, P(rate_lane), None), "get_source_rates")
        p1, w1 = sim.network_stats()
        assert p1 - p0 == 1 and w1 - w0 >= 2      # the host pass ran
        G_lane, R_lane = sim.source_network()
        sim.set_network_walk("wave")      # after the network is set
        assert sim.network_pass() == ("device", "device") and sim.network_walk() == ("wave", "wave")
        check_wave_pass(sim, lm, c)      # the host pass' bits (carries the sources again)
        assert sim.pre_eval(0.0, y) == 0
        rate = np.zeros(n)
        sim._chk(wl.LIB.wai_get_source_rates(sim.h, P(rate), None), "get_source_rates")      # (the description's upload: one wait, once)
        p0, w0 = sim.network_stats()
        sim._chk(wl.LIB.wai_get_source_rates(sim.h, P(rate), None), "get_source_rates")
        p1, w1 = sim.network_stats()
        assert p1 - p0 == 1 and w1 - w0 == 0      # the pass ran on the device: nobody waited
        G, R = sim.source_network()
        assert abs(G[0, 0] + 0.3 * 450) < 1e-9 and R[0, 0] > 0      # the limit and the reinjector are at work
        assert same_bits(rate, rate_lane) and same_bits(G, G_lane) and same_bits(R, R_lane)
    finally:
        sim.set_network_walk("wave")


def test_network_above_160_kib_keeps_the_host_pass(wave):
    sim, lm = wave
    c = wc.flat_behind_limit(800)
    carry(sim, lm, c)
    limit, needed = lds(sim)
    assert limit == wc.WAVE_LDS_DOUBLES and needed == wc.schedule(c["spec"])["lds"][0] > limit
    assert sim.network_pass() == ("device", "host") and sim.network_walk() == ("wave", "lane")
    with pytest.raises(wl.WaiError) as e:
        device_pass(sim, c)
    assert "needs 180272 bytes of LDS" in str(e.value)
    assert sim.pre_eval(0.0, small_state()) == 0
    rate = np.zeros(len(c["rate"]))
    p0, w0 = sim.network_stats()
    sim._chk(wl.LIB.wai_get_source_rates(sim.h, P(rate), None), "get_source_rates")
    p1, w1 = sim.network_stats()
    assert p1 - p0 == 1 and w1 - w0 >= 2      # the host pass ran
    G, R = sim.source_network()
    assert abs(G[0, 0] + 0.3 * 800) < 1e-9


@pytest.mark.parametrize("name", ["source", "group"])
def test_refused_topology_keeps_the_lane_walk(wave, name):
    """a source in two groups, a group under two groups: the lane walk stays in force, with the host pass' bits"""
    sim, lm = wave
    c = dict(source=wc.source_in_two_groups, group=wc.group_under_two_groups)[name]()
    check_pass(sim, lm, c)
    assert sim.network_walk() == ("wave", "lane") and sim.network_pass() == ("device", "device")
    assert lds(sim)[0] == 8192


def test_unknown_walk_is_refused(wave):
    sim, lm = wave
    with pytest.raises(wl.WaiError) as e:
        sim._chk(wl.LIB.wai_set_network_walk(sim.h, 2), "set_network_walk")
    assert "(-2)" in str(e.value) and "WAI_NETWORK_WALK_WAVE" in str(e.value)
    with pytest.raises(ValueError):
        sim.set_network_walk("sideways")
    assert sim.network_walk()[0] == "wave"
