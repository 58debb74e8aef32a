"""Source networks for the tests of the flat pass (csrc/network_pass.hpp: tests/test_network_pass_host.py on the host,
tests/test_hip_network_device.py on the device).  A case is dict(spec, rate, enth, sep): the description of
lib.network_arrays, the sources' own rates and flowing enthalpies, and their separators (8 doubles each).

The oracle of the host tests is tests/golden/network_pass_bits.json: what wai_network_evaluate gave for every case while the
library still had a second, recursive pass on a network of structs (the commit the file names) -- today the library's host
pass is network_pass itself, so comparing the two would compare a text with itself.  The specified enthalpies of a case
are the flowing ones handed in."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HF, HG = 6.7e5, 2.75e6   # a separator at about 6 bar


def case(spec, rate, enth, sep=None):
    n = len(rate)
    return dict(spec=spec, rate=np.asarray(rate, dtype=float), enth=np.asarray(enth, dtype=float),
                sep=np.zeros(8 * n) if sep is None else np.asarray(sep, dtype=float))


def separators(n, which, stages=((HF, HG),)):
    sep = np.zeros(8 * n)
    for i in which:
        for q, (hf, hg) in enumerate(stages):
            sep[8 * i + 2 * q], sep[8 * i + 2 * q + 1] = hf, hg
    return sep


def reference_fixture(sep_enth):
    """the reference's reinjector unit test: 39 sources, 6 groups, 10 reinjectors (tests/test_network.py)"""
    from waiwera_amd.simulation import network_spec
    inp = json.load(open(os.path.join(HERE, "golden", "inputs", "test_source_network_reinjector.json")))
    fx = json.load(open(os.path.join(HERE, "golden", "reference_unit_values_network.json")))
    spec, names, timed = network_spec(inp, fx["interval"], sep_enth)
    sources = inp["source"]
    n = len(sources)
    rate = np.array([float(s.get("rate", 0.0)) for s in sources])
    enth = np.array([fx["production_enthalpy"].get(s["name"], 0.0) for s in sources])
    sep = np.zeros(8 * n)
    for i, s in enumerate(sources):
        if s.get("separator"):
            sep[8 * i], sep[8 * i + 1] = sep_enth(s["separator"]["pressure"])
    assert (n, len(spec["groups"]), len(spec["reinjectors"])) == (39, 6, 10)
    return case(spec, rate, enth, sep)


def three_wells(scaling):
    """the uniform / progressive limiter cases of tests/test_network.py"""
    spec = dict(rate_specified=[1, 1, 1], enthalpy_specified=[0, 0, 0], reinjectors=[],
                groups=[dict(inputs=[(1, 0), (1, 1), (1, 2)], scaling=scaling, limits=[(0, 6.0)], separator=None)])
    return case(spec, [-4.0, -3.0, -2.0], [1.0e6, 1.0e6, 1.0e6])


def nested(outer_limit=7.0):
    """groups nested three deep: a progressive total limit at the outer level, a progressive group between, and a uniform
    group with a steam limit of its own inside"""
    n = 6
    spec = dict(rate_specified=[1] * n, enthalpy_specified=[0] * n, reinjectors=[], groups=[
        dict(inputs=[(1, 0), (1, 1)], scaling=0, limits=[(2, 0.9)], separator=None),
        dict(inputs=[(1, 2), (2, 0), (1, 3)], scaling=1, limits=[], separator=None),
        dict(inputs=[(1, 4), (2, 1), (1, 5)], scaling=1, limits=[(0, outer_limit), (1, 5.5)], separator=None)])
    return case(spec, [-3.1, -2.3, -1.7, -0.9, -1.3, -2.9], [1.1e6, 1.4e6, 0.9e6, 1.2e6, 1.0e6, 1.3e6], separators(n, range(n)))


def separated_limit(flow, scaling):
    """a limit on water (1) or steam (2) behind a group's own two-stage separator"""
    n = 4
    spec = dict(rate_specified=[1] * n, enthalpy_specified=[0] * n, reinjectors=[], groups=[
        dict(inputs=[(1, i) for i in range(n)], scaling=scaling, limits=[(flow, 1.25)],
             separator=[(HF, HG), (4.2e5, 2.68e6)])])
    return case(spec, [-2.5, -1.5, -3.5, -0.5], [1.2e6, 1.5e6, 1.0e6, 2.9e6])


def chain(rates=(-6.0, -4.0, 0.0, 1.5, 0.0, 0.0)):
    """a reinjector chain: a proportion output, an unrated output onto a source with a rate of its own, a rate output to a
    second reinjector, an overflow source; the second reinjector overflows to a third, which is fed by nothing else"""
    n = 7
    spec = dict(rate_specified=[1, 1, 0, 1, 0, 0, 0], enthalpy_specified=[0, 0, 0, 1, 0, 0, 0],
                groups=[dict(inputs=[(1, 0), (1, 1)], scaling=0, limits=[(0, 9.0)], separator=[(HF, HG)])],
                reinjectors=[
                    dict(input=(2, 0), overflow=(1, 4), outputs=[
                        dict(flow=1, out=(1, 2), rate=-1.0, proportion=0.35, enthalpy=-1.0),
                        dict(flow=1, out=(1, 3), rate=-1.0, proportion=-1.0, enthalpy=-1.0),
                        dict(flow=2, out=(3, 1), rate=0.4, proportion=-1.0, enthalpy=-1.0),
                        dict(flow=1, out=(3, 1), rate=-1.0, proportion=0.2, enthalpy=4.4e5)]),
                    dict(input=(0, -1), overflow=(3, 2), outputs=[
                        dict(flow=2, out=(1, 5), rate=0.1, proportion=-1.0, enthalpy=-1.0),
                        dict(flow=1, out=(0, -1), rate=0.05, proportion=-1.0, enthalpy=-1.0)]),
                    dict(input=(0, -1), overflow=(0, -1), outputs=[
                        dict(flow=1, out=(1, 6), rate=-1.0, proportion=-1.0, enthalpy=-1.0)])])
    r = list(rates) + [0.0]
    return case(spec, r, [1.3e6, 1.1e6, 0.0, 3.0e5, 0.0, 0.0, 0.0], separators(n, [0]))


def signs():
    """zero and positive totals: the q < 0 branches not taken (no separation, no separated sums)"""
    out = []
    for rates in ([0.0, 0.0, 0.0], [2.0, 5.0, 1.0], [-1.0, 1.0, 0.0], [-0.0, 0.0, -0.0]):
        spec = dict(rate_specified=[1, 1, 1], enthalpy_specified=[0, 0, 0],
                    groups=[dict(inputs=[(1, 0), (1, 1)], scaling=1, limits=[(0, 3.0)], separator=[(HF, HG)]),
                            dict(inputs=[(2, 0), (1, 2)], scaling=0, limits=[(0, 4.0)], separator=None)],
                    reinjectors=[dict(input=(2, 1), overflow=(0, -1), outputs=[])])
        out.append(case(spec, rates, [1.0e6, 1.2e6, 0.8e6], separators(3, [0, 1, 2])))
    return out


def random_network(seed):
    """a seeded network of at most 12 sources, 4 groups and 4 reinjectors: every source and group is taken in at most once;
    reinjectors deliver to injection sources, to later reinjectors or to nobody"""
    rng = np.random.default_rng(seed)
    n_prod, n_inj = int(rng.integers(1, 8)), int(rng.integers(1, 6))
    n = n_prod + n_inj
    rate = np.concatenate([-rng.uniform(0.0, 5.0, n_prod) * (rng.random(n_prod) > 0.15), rng.uniform(0.0, 3.0, n_inj) * (rng.random(n_inj) > 0.3)])
    enth = np.concatenate([rng.uniform(4.0e5, 3.0e6, n_prod), rng.uniform(8.0e4, 5.0e5, n_inj)])
    sep = np.zeros(8 * n)
    for i in range(n_prod):
        if rng.random() < 0.6:
            stages = [(HF, HG), (4.2e5, 2.68e6), (3.0e5, 2.6e6)][: int(rng.integers(1, 4))]
            sep[8 * i: 8 * i + 2 * len(stages)] = np.ravel(stages)
    free = [(1, i) for i in range(n_prod)]   # nodes no group has taken in yet
    groups = []
    for g in range(int(rng.integers(0, 5))):
        if not free:
            break
        k = int(rng.integers(1, min(len(free), 4) + 1))
        pick = [free.pop(int(rng.integers(0, len(free)))) for _ in range(k)]
        total = sum(abs(rate[i]) for kind, i in pick if kind == 1) + 1.0
        limits = [(int(rng.integers(0, 3)), float(rng.uniform(0.1, 1.2) * total)) for _ in range(int(rng.integers(0, 3)))]
        limits = list({t: (t, v) for t, v in limits}.values())
        groups.append(dict(inputs=pick, scaling=int(rng.integers(0, 2)), limits=limits,
                           separator=[(HF, HG)] if rng.random() < 0.4 else None))
        free.append((2, g))
    nr = int(rng.integers(0, 5))
    inj = list(range(n_prod, n))
    rng.shuffle(inj)
    reinj = []
    for r in range(nr):
        outs = []
        for _ in range(int(rng.integers(0, 4))):
            u = rng.random()
            if u < 0.55 and inj:
                out = (1, int(inj.pop()))
            elif u < 0.8 and r + 1 < nr:
                out = (3, int(rng.integers(r + 1, nr)))
            else:
                out = (0, -1)
            mode = int(rng.integers(0, 3))
            outs.append(dict(flow=int(rng.integers(1, 3)), out=out, rate=float(rng.uniform(0.0, 2.0)) if mode == 0 else -1.0,
                             proportion=float(rng.uniform(0.0, 0.8)) if mode == 1 else -1.0,
                             enthalpy=float(rng.uniform(1.0e5, 5.0e5)) if rng.random() < 0.3 else -1.0))
        u = rng.random()
        over = (1, int(inj.pop())) if u < 0.3 and inj else ((3, int(rng.integers(r + 1, nr))) if u < 0.6 and r + 1 < nr else (0, -1))
        src = free[int(rng.integers(0, len(free)))] if free and rng.random() < 0.75 else (0, -1)
        reinj.append(dict(input=src, overflow=over, outputs=outs))
    spec = dict(rate_specified=[int(rng.random() < 0.6) for _ in range(n)], enthalpy_specified=[int(rng.random() < 0.3) for _ in range(n)],
                groups=groups, reinjectors=reinj)
    return case(spec, rate, enth, sep)


def fed_sources(spec):
    """the sources a reinjector delivers or overflows to"""
    fed = set()
    for r in spec["reinjectors"]:
        fed |= {o["out"][1] for o in r["outputs"] if o["out"][0] == 1}
        if r["overflow"][0] == 1:
            fed.add(r["overflow"][1])
    return sorted(fed)


def handed_over(c, S):
    """what network_update hands the device after a pass with source states S: ((mode, value) pairs (n, 2), fed sources,
    their enthalpies) -- mode 2 with the output rate for fed sources, mode 1 with rate / raw where the rate changed, else 0"""
    n = len(c["rate"])
    fed = fed_sources(c["spec"])
    net = np.zeros((n, 2))
    for i in range(n):
        raw = c["rate"][i]
        if i in fed:
            net[i] = (2.0, S[i, 0])
        elif S[i, 0] != raw:
            net[i] = (1.0, S[i, 0] / raw if raw != 0.0 else 1.0)
    return net, fed, S[fed, 1]


def with_sources(c, n):
    """case c with extra producers up to n sources in all (the lane-strided loops' edges)"""
    extra = n - len(c["rate"])
    assert extra >= 0
    n0 = len(c["rate"])
    k = np.arange(extra)
    # ... behind a uniform limit of their own, so that every one of them gets a factor
    more = [dict(inputs=[(1, n0 + int(i)) for i in k], scaling=0, limits=[(0, 0.1 * extra)], separator=None)] if extra else []
    spec = dict(c["spec"], rate_specified=list(c["spec"]["rate_specified"]) + [0] * extra,
                enthalpy_specified=list(c["spec"]["enthalpy_specified"]) + [0] * extra, groups=list(c["spec"]["groups"]) + more)
    return case(spec, np.concatenate([c["rate"], -0.25 * (1 + k % 3)]), np.concatenate([c["enth"], 9.0e5 + 1.0e4 * k]),
                np.concatenate([c["sep"], separators(extra, range(0, extra, 2))]))


# ---- the recorded bits ----------------------------------------------------------------------------------------------
_RECORDED = {}


def recorded(name):
    if not _RECORDED:
        _RECORDED.update(json.load(open(os.path.join(HERE, "golden", "network_pass_bits.json")))["cases"])
    return _RECORDED[name]


def _digest(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a, dtype="<f8").tobytes() for a in arrays)).hexdigest()


def on_recorded_inputs(c, name="reference_fixture"):
    """case c with the numeric inputs the bits of `name` were recorded on (separator enthalpies come out of the oracle's
    libm: the same formulas elsewhere may differ in the last place), after checking that c's own agree with them"""
    out = dict(c)
    for key, hexes in recorded(name)["inputs"].items():
        out[key] = np.array([float.fromhex(x) for x in hexes])
        assert out[key].shape == c[key].shape, (name, key)
        # 1e-12 relative: the same formulas through a possibly different libm
        assert np.all(np.abs(out[key] - c[key]) <= 1e-12 * np.abs(out[key])), (name, key, out[key], c[key])
    return out


def assert_recorded(name, c, S, G, R, who):
    """the node states (sources, groups, reinjectors) `who` gave for case c are the recorded ones, bit for bit"""
    rec = recorded(name)
    assert _digest(c["rate"], c["enth"], c["sep"]) == rec["inputs_sha256"], \
        "%s: the case's numeric inputs are not the ones its bits were recorded on -- the generator drifted, not the pass" % name
    got = np.concatenate([np.ravel(np.asarray(x, dtype=float)) for x in (S, G, R)])
    if "hex" in rec:
        want = np.array([float.fromhex(x) for x in rec["hex"]])
        assert got.shape == want.shape, (name, who, got.shape, want.shape)
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, "%s: %s differs from the recorded bits at doubles %s: %s, recorded %s" % (
            name, who, bad[:8], [float(x).hex() for x in got[bad[:8]]], [rec["hex"][i] for i in bad[:8]])
    else:
        assert _digest(got) == rec["sha256"], "%s: %s differs from the recorded bits (digest of %d doubles)" % (name, who, got.size)
