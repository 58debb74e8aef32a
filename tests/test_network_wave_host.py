"""The source network's wave-wide walk (waiwera_amd/csrc/network_wave.hpp) without a GPU: a stand-alone program
(tests/network_wave_host/main.cpp) built with the address and undefined-behaviour sanitizers builds the flat description and
the wave schedule from a text file and runs network_pass_wave -- the text the wave kernels run -- over 64 emulated lanes three
times: lanes ascending, descending and in a seeded shuffle.

The three runs must print the same bits (a difference is a race between the lanes of one phase), and those bits must be the
recorded ones of tests/golden/network_pass_bits.json (the library's former recursive host pass; tests/network_cases.py), as
must those of the library's host pass, wai_network_evaluate (the lane walk's network_pass; the library is only loaded):
node states of sources, groups and reinjectors, then the (mode, value) pairs and the fed sources' enthalpies by the
hand-over rule on those states.  The schedule is checked against a construction from its definition
(tests/network_wave_cases.py), the refusals with their texts, the switch's values, names and defaults without a device."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import network_cases as nc
from tests import network_wave_cases as wc
from tests.test_network_pass_host import CHAINS, ENTH_IN, same_bits, write_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ("ascending", "descending", "shuffled")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("network_wave_host") / "network_wave_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "network_wave_host", "main.cpp"), "-o", str(exe)])
    return str(exe)


def run(program, path, seed=7):
    p = subprocess.run([program, str(path), str(seed)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = {}
    for line in p.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name in ("error", "refused"):
            code, _, text = rest.partition(" ")
            assert int(code) == -2
            return {name: text}
        out[name] = (np.array([int(x) for x in rest.split()], dtype=int) if name.startswith("schedule.")
                     else np.array([float.fromhex(x) for x in rest.split()]))
    return out


def check(program, tmp_path, c, name, seed=7):
    """case c, recorded under `name`"""
    from waiwera_amd import lib as wl
    tag = re.sub(r"\W+", "_", name)
    path = tmp_path / (tag + ".txt")
    write_case(path, c)
    got = run(program, path, seed)
    assert "error" not in got and "refused" not in got, got
    S, G, R = wl.network_evaluate(c["spec"], c["rate"], c["enth"], c["sep"])
    nc.assert_recorded(name, c, S, G, R, "wai_network_evaluate")
    for order in ORDERS:
        nc.assert_recorded(name, c, *(got["%s.%s" % (k, order)] for k in ("sources", "groups", "reinjectors")),
                           "the wave walk, lanes " + order)
    net, fed, enth = nc.handed_over(c, S)
    want_enth = np.full(len(c["rate"]), ENTH_IN)
    want_enth[fed] = enth
    for order in ORDERS:      # the recorded bits in every lane order: then the three are the same bits too
        for name, want in (("sources", S), ("groups", G), ("reinjectors", R), ("net", net), ("enth", want_enth)):
            have = got["%s.%s" % (name, order)]
            assert same_bits(have, want), (tag, order, name, np.argwhere(have != np.ravel(want))[:8].ravel())
            assert same_bits(have, got["%s.%s" % (name, ORDERS[0])]), (tag, order, name, "the lane orders differ")
    sch = wc.schedule(c["spec"])
    for name in ("ds_ptr", "ds", "dg_ptr", "dg", "an_ptr", "an", "gc_ptr", "gc", "out_shared", "fan_in", "stage", "lds"):
        assert np.array_equal(got["schedule." + name], sch[name]), (tag, name, got["schedule." + name], sch[name])
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
    assert np.count_nonzero(got["net.ascending"].reshape(-1, 2)[:, 0] == 2.0) == len(nc.fed_sources(c["spec"])) > 0
    for n in (63, 64, 65, 130):
        check(program, tmp_path, nc.with_sources(c, n), "with_sources(reference_fixture,%d)" % n)


def test_cases_of_the_lane_walk(program, tmp_path):
    """every hand-made case of tests/network_cases.py"""
    cases = [("three_wells(%d)" % s, nc.three_wells(s)) for s in (0, 1)] + [("nested(%g)" % o, nc.nested(o)) for o in (7.0, 3.0, 100.0)]
    cases += [("separated_limit(%d,%d)" % (f, s), nc.separated_limit(f, s)) for f in (1, 2) for s in (0, 1)]
    cases += [("chain(%d)" % k, nc.chain(r)) for k, r in enumerate(CHAINS)]
    cases += [("signs(%d)" % k, c) for k, c in enumerate(nc.signs())]
    assert len(cases) == 16
    for name, c in cases:
        check(program, tmp_path, c, name)


def test_random_networks_of_the_lane_walk(program, tmp_path):
    """the 200 seeded networks of tests/test_network_pass_host.py: none is refused"""
    for seed in range(200):
        check(program, tmp_path, nc.random_network(seed), "random_network(%d)" % seed, seed)


@pytest.mark.parametrize("scaling", [0, 1])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
def test_wide_groups_at_the_staging_loops_edges(program, tmp_path, m, scaling):
    c = wc.wide_group(m, scaling)
    got = check(program, tmp_path, c, "wide_group(%d,%d)" % (m, scaling))
    S = got["sources.ascending"].reshape(m, 6)
    assert got["schedule.fan_in"][0] == m and got["schedule.stage"][0] == 8 + 6 * m
    assert not same_bits(S[:, 0], c["rate"])      # the limit is at work
    if scaling == 1 and m > 1:      # progressive: untouched before the break, cut at it, shut behind it
        b = {65: 64, 130: 100}.get(m, m // 2)
        assert same_bits(S[:b, 0], c["rate"][:b]) and 0 < abs(S[b, 0]) < abs(c["rate"][b]) and np.all(S[b + 1:, 0] == 0.0)
        assert b >= 64 or m < 65


@pytest.mark.parametrize("outer", [20.0, 6.0, 1000.0])
def test_nested_three_deep_with_a_wide_inner_group(program, tmp_path, outer):
    got = check(program, tmp_path, wc.nested_wide(70, outer), "nested_wide(70,%g)" % outer)
    assert list(got["schedule.an"]) == [1, 2, 2] and list(got["schedule.dg"]) == [0, 0, 1]
    assert abs(got["groups.ascending"].reshape(3, 6)[0, 4]) <= 3.0 * (1 + 1e-12)      # the inner steam limit holds


def test_reinjector_with_65_outputs_and_an_overflow(program, tmp_path):
    c = wc.wide_reinjector(65)
    got = check(program, tmp_path, c, "wide_reinjector(65)")
    assert got["schedule.fan_in"][0] == 65 and not got["schedule.out_shared"].any()
    R = got["reinjectors.ascending"].reshape(1, 8)
    assert R[0, 0] > 0 and R[0, 1] > 0 and R[0, 2] > 0      # water and steam delivered, and something left for the overflow


def test_two_outputs_onto_one_source_are_delivered_in_order(program, tmp_path):
    """the wave walk does not refuse them: the schedule flags every output onto a source with more than one writer, and the
    lane that runs the balance chain delivers those in output order"""
    c = wc.two_outputs_one_source()
    got = check(program, tmp_path, c, "two_outputs_one_source")
    assert list(got["schedule.out_shared"]) == [1, 0, 1, 0]


def test_wide_random_networks(program, tmp_path):
    """120 seeded networks of at most 200 sources, 6 groups and 4 reinjectors"""
    seen = dict(groups=0, reinj=0, limited=0, progressive=0, nested=0, wide=0, shared=0)
    for seed in range(120):
        c = wc.wide_random(seed)
        spec = c["spec"]
        assert len(c["rate"]) <= 200 and len(spec["groups"]) <= 6 and len(spec["reinjectors"]) <= 4
        got = check(program, tmp_path, c, "wide_random(%d)" % seed, seed)
        seen["groups"] += bool(spec["groups"])
        seen["reinj"] += bool(spec["reinjectors"])
        seen["limited"] += any(g["limits"] for g in spec["groups"])
        seen["progressive"] += any(g["limits"] and g["scaling"] for g in spec["groups"])
        seen["nested"] += any(k == 2 for g in spec["groups"] for k, _ in g["inputs"])
        seen["wide"] += got["schedule.fan_in"][0] > 64
        seen["shared"] += bool(got["schedule.out_shared"].any())
    assert min(seen.values()) >= 40, seen   # the generator reaches every part of the walk


@pytest.mark.parametrize("name,text", [("source", "network wave walk: source 1 is taken in more than once"),
                                       ("group", "network wave walk: group 0 is taken in more than once"),
                                       ("lds", "network wave walk: needs 180272 bytes of LDS, a workgroup has 163840")])
def test_refusals(program, tmp_path, name, text):
    c = dict(source=wc.source_in_two_groups, group=wc.group_under_two_groups, lds=lambda: wc.flat_behind_limit(800))[name]()
    path = tmp_path / "refused.txt"
    write_case(path, c)
    assert run(program, path) == {"refused": text}
    if name == "lds":
        assert 8 * wc.schedule(c["spec"])["lds"][0] == 180272 > 8 * wc.WAVE_LDS_DOUBLES
        near = wc.schedule(wc.flat_behind_limit(450)["spec"])
        assert 8192 < near["lane_lds"] and near["lds"][0] < wc.WAVE_LDS_DOUBLES      # what only the wave walk holds on the device


def test_switch_defaults_without_a_device():
    """the ABI's values, the bindings' names and the front ends' defaults: the lane walk unless asked otherwise"""
    from waiwera_amd import lib as wl
    from waiwera_amd import run as wr
    from waiwera_amd.flow_simulation import FlowSimulation
    from waiwera_amd.simulation import Simulation
    hdr = open(os.path.join(ROOT, "include", "waiwera_hip.h")).read()
    assert re.search(r"enum\s*{\s*WAI_NETWORK_WALK_LANE\s*=\s*0\s*,\s*WAI_NETWORK_WALK_WAVE\s*=\s*1\s*}", hdr)
    assert wl.NETWORK_WALK == {"lane": 0, "wave": 1}
    for name in ("wai_set_network_walk", "wai_get_network_walk"):
        assert name in wl.EXPORTED and re.search(r"\bint\s+%s\s*\(" % name, hdr)
    assert inspect.signature(Simulation.__init__).parameters["network_walk"].default == "lane"
    assert hasattr(FlowSimulation, "set_network_walk") and hasattr(FlowSimulation, "network_walk")
    with pytest.raises(ValueError):
        Simulation({}, network_walk="sideways")
    src = inspect.getsource(wr.main)
    assert re.search(r'"--network-walk", choices=\("lane", "wave"\), default="lane"', src), "python -m waiwera_amd.run --network-walk lane|wave"
    with pytest.raises(SystemExit):
        wr.main(["input.json", "--network-walk", "sideways"])
    f90 = open(os.path.join(ROOT, "waiwera_amd", "fortran", "waiwera_hip_module.F90")).read()
    assert re.search(r"WAI_NETWORK_WALK_LANE\s*=\s*0\s*,\s*WAI_NETWORK_WALK_WAVE\s*=\s*1", f90)
    assert re.search(r"procedure, public :: set_network_walk\b", f90)
