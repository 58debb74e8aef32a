"""The source network's pass on its flat description (waiwera_amd/csrc/network_pass.hpp) without a GPU: a stand-alone
program (tests/network_pass_host/main.cpp) built with the address and undefined-behaviour sanitizers builds the description
from a text file, runs network_pass -- the text k_network_pass runs on the device -- and prints every double in hex.

The oracle is tests/golden/network_pass_bits.json: the node states of sources and groups (6 doubles each) and reinjectors
(8 each) that the library's former recursive host pass gave for every case here, recorded before it was deleted.  The
program's states AND those of the library's host pass, wai_network_evaluate (the same network_pass, built into the library;
only loaded), must equal them BIT FOR BIT, and the (mode, value) pairs and enthalpies the pass hands the residual kernel
must follow the hand-over rule (tests/network_cases.py, handed_over) on those states."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import network_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rate_specified enthalpy_specified grp_ptr grp_in_kind grp_in grp_scaling grp_limit_type grp_limit grp_sep rj_in_kind rj_in "
         "rj_out_ptr out_flow out_kind out_node out_rate out_proportion out_enthalpy rj_overflow_kind rj_overflow").split()
ENTH_IN = -12345.0   # what the pass must leave in the enthalpy array of sources nobody feeds


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("network_pass_host") / "network_pass_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "network_pass_host", "main.cpp"), "-o", str(exe)])
    return str(exe)


def write_case(path, c):
    from waiwera_amd import lib as wl
    spec = c["spec"]
    keep, _ = wl.network_arrays(spec)
    n, ng, nr = len(c["rate"]), len(spec["groups"]), len(spec["reinjectors"])
    recs = dict(zip(NAMES, keep))
    recs.update(n=[n], n_groups=[ng], n_reinj=[nr], src_sep=c["sep"], src_enth0=c["enth"],
                raw=np.concatenate([c["rate"], c["enth"]]), enth_in=np.full(n, ENTH_IN))
    # (arrays of an absent part are one placeholder long in network_arrays: cut to what the counts say)
    n_in = int(recs["grp_ptr"][ng]) if ng else 0
    n_out = int(recs["rj_out_ptr"][nr]) if nr else 0
    size = dict(grp_in_kind=n_in, grp_in=n_in, grp_scaling=ng, grp_limit_type=3 * ng, grp_limit=3 * ng, grp_sep=8 * ng, rj_in_kind=nr,
                rj_in=nr, out_flow=n_out, out_kind=n_out, out_node=n_out, out_rate=n_out, out_proportion=n_out, out_enthalpy=n_out,
                rj_overflow_kind=nr, rj_overflow=nr)
    with open(path, "w") as f:
        for name, v in recs.items():
            v = np.atleast_1d(np.asarray(v))[: size.get(name)]
            txt = [float(x).hex() for x in v] if v.dtype.kind == "f" else [str(int(x)) for x in v]
            f.write("%s %d %s\n" % (name, len(txt), " ".join(txt)))


def run(program, path):
    p = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = {}
    for line in p.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "error":
            code, _, text = rest.partition(" ")
            assert int(code) == -2
            return {"error": text}
        out[name] = np.array([int(x) for x in rest.split()]) if name == "sizes" else np.array([float.fromhex(x) for x in rest.split()])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check(program, tmp_path, c, name):
    """case c, recorded under `name`: the program and the library against the recorded bits, then the hand-over"""
    from waiwera_amd import lib as wl
    tag = re.sub(r"\W+", "_", name)
    path = tmp_path / (tag + ".txt")
    write_case(path, c)
    got = run(program, path)
    assert "error" not in got, got
    nc.assert_recorded(name, c, got["sources"], got["groups"], got["reinjectors"], "the stand-alone program")
    S, G, R = wl.network_evaluate(c["spec"], c["rate"], c["enth"], c["sep"])
    nc.assert_recorded(name, c, S, G, R, "wai_network_evaluate")
    net, fed, enth = nc.handed_over(c, S)
    assert same_bits(got["net"], net), (tag, got["net"].reshape(-1, 2), net)
    want = np.full(len(c["rate"]), ENTH_IN)
    want[fed] = enth
    assert same_bits(got["enth"], want), (tag, got["enth"], want)
    return got


def test_reference_reinjector_fixture(program, tmp_path, oracle):
    import ctypes as C
    from oracle import binding as ol
    e = ol.Eos()
    oracle.wo_eos_init(C.byref(e), 1)

    def sep_enth(p):
        hf, hg = np.zeros(1), np.zeros(1)
        assert oracle.wo_separator_enthalpies(C.byref(e), float(p), ol.dp(hf), ol.dp(hg)) == 0
        return float(hf[0]), float(hg[0])
    c = nc.on_recorded_inputs(nc.reference_fixture(sep_enth))
    got = check(program, tmp_path, c, "reference_fixture")
    assert np.count_nonzero(got["net"].reshape(-1, 2)[:, 0] == 2.0) == len(nc.fed_sources(c["spec"])) > 0


@pytest.mark.parametrize("scaling", [0, 1])
def test_three_well_limiters(program, tmp_path, scaling):
    got = check(program, tmp_path, nc.three_wells(scaling), "three_wells(%d)" % scaling)
    assert np.allclose(got["sources"].reshape(3, 6)[:, 0], [[-4.0 * 6 / 9, -3.0 * 6 / 9, -2.0 * 6 / 9], [-4.0, -2.0, 0.0]][scaling], atol=1e-12)


@pytest.mark.parametrize("outer", [7.0, 3.0, 100.0])
def test_nested_three_deep(program, tmp_path, outer):
    """a progressive limit outside, a progressive group between, a uniform limit inside: the explicit stack and the arena of
    node_limit tables against the recorded recursion (outer 3.0 cuts into the inner groups, 100.0 leaves the outer limit idle)"""
    c = nc.nested(outer)
    got = check(program, tmp_path, c, "nested(%g)" % outer)
    n_iw, n_dw, frames, arena, lds = got["sizes"]
    assert frames == 2 * 3 + 2 and arena == 3 + 9 + 9   # three levels; the outer and the middle group's tables [3][3]
    if outer < 100.0:
        assert abs(got["groups"].reshape(3, 6)[2, 0]) <= outer * (1 + 1e-12)


@pytest.mark.parametrize("flow", [1, 2])
@pytest.mark.parametrize("scaling", [0, 1])
def test_limit_behind_group_separator(program, tmp_path, flow, scaling):
    got = check(program, tmp_path, nc.separated_limit(flow, scaling), "separated_limit(%d,%d)" % (flow, scaling))
    if scaling == 0:   # one factor for every member scales the separated flows with the total: the limit is met exactly.
        # (progressive scaling shares the limit out by the MEMBERS' separated flows, which these wells without separators of
        # their own do not have: the oracle's bits are the check there)
        assert abs(got["groups"].reshape(1, 6)[0, 2 * flow]) <= 1.25 * (1 + 1e-12)


CHAINS = [(-6.0, -4.0, 0.0, 1.5, 0.0, 0.0), (-6.0, -4.0, 0.0, 0.2, 0.0, 0.0), (0.0, 0.0, 0.0, 1.5, 0.0, 0.0)]


@pytest.mark.parametrize("rates", CHAINS)
def test_reinjector_chain(program, tmp_path, rates):
    """proportion, unrated and rate outputs, an output to a second reinjector, overflow to a source and down the chain"""
    got = check(program, tmp_path, nc.chain(rates), "chain(%d)" % CHAINS.index(rates))
    assert list(np.flatnonzero(got["net"].reshape(-1, 2)[:, 0] == 2.0)) == [2, 3, 4, 5, 6]


def test_zero_and_positive_totals(program, tmp_path):
    for k, c in enumerate(nc.signs()):
        check(program, tmp_path, c, "signs(%d)" % k)


def test_random_networks(program, tmp_path):
    """200 seeded networks of at most 12 sources, 4 groups and 4 reinjectors"""
    seen = dict(groups=0, reinj=0, limited=0, progressive=0, nested=0)
    for seed in range(200):
        c = nc.random_network(seed)
        spec = c["spec"]
        assert len(c["rate"]) <= 12 and len(spec["groups"]) <= 4 and len(spec["reinjectors"]) <= 4
        check(program, tmp_path, c, "random_network(%d)" % seed)
        seen["groups"] += bool(spec["groups"])
        seen["reinj"] += bool(spec["reinjectors"])
        seen["limited"] += any(g["limits"] for g in spec["groups"])
        seen["progressive"] += any(g["limits"] and g["scaling"] for g in spec["groups"])
        seen["nested"] += any(k == 2 for g in spec["groups"] for k, _ in g["inputs"])
    assert min(seen.values()) >= 40, seen   # the generator reaches every part of the pass


def test_cyclic_reinjectors_are_refused(program, tmp_path):
    c = nc.chain()
    c["spec"]["reinjectors"][2]["overflow"] = (3, 0)
    path = tmp_path / "cycle.txt"
    write_case(path, c)
    assert run(program, path) == {"error": "source network reinjectors form a cycle"}
    from waiwera_amd import lib as wl
    with pytest.raises(wl.WaiError):   # the library refuses it too (the same builder serves both)
        wl.network_evaluate(c["spec"], c["rate"], c["enth"], c["sep"])


def test_switch_defaults_without_a_device():
    """the ABI's values, the bindings' names and the front ends' defaults: the host pass unless asked otherwise"""
    from waiwera_amd import lib as wl
    from waiwera_amd import run as wr
    from waiwera_amd.flow_simulation import FlowSimulation
    from waiwera_amd.simulation import Simulation
    hdr = open(os.path.join(ROOT, "include", "waiwera_hip.h")).read()
    assert re.search(r"enum\s*{\s*WAI_NETWORK_PASS_HOST\s*=\s*0\s*,\s*WAI_NETWORK_PASS_DEVICE\s*=\s*1\s*}", hdr)
    assert wl.NETWORK_PASS == {"host": 0, "device": 1}
    for name in ("wai_set_network_pass", "wai_get_network_pass", "wai_test_network_pass", "wai_test_network_stats"):
        assert name in wl.EXPORTED
    assert inspect.signature(Simulation.__init__).parameters["network_pass"].default == "host"
    assert hasattr(FlowSimulation, "set_network_pass") and hasattr(FlowSimulation, "network_pass")
    with pytest.raises(ValueError):
        Simulation({}, network_pass="elsewhere")
    src = inspect.getsource(wr.main)
    m = re.search(r'"--network-pass", choices=\("host", "device"\), default="host"', src)
    assert m, "python -m waiwera_amd.run --network-pass host|device, default host"
    with pytest.raises(SystemExit):
        wr.main(["input.json", "--network-pass", "elsewhere"])
