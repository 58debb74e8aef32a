"""Source networks for the tests of the wave-wide walk (csrc/network_wave.hpp: tests/test_network_wave_host.py on the host,
tests/test_hip_network_wave.py on the device), beside those of tests/network_cases.py, whose form they share: a case is
dict(spec, rate, enth, sep).  Wide fan-ins at the edges of the lanes' staging loops, and the wave schedule built in Python
from its definition."""
import numpy as np

from tests import network_cases as nc

LANES = 64
STAGE = 6                  # staged doubles per input
CTL = 8                    # doubles at the head of the staging run that carry a phase's results to the next
WAVE_LDS_DOUBLES = 20480   # 160 KiB


def producers(n, k0=0):
    """rates, enthalpies and separators (on two of three) of n producers"""
    k = np.arange(k0, k0 + n)
    return -0.25 * (1 + k % 3) - 0.001 * (k % 11), 9.0e5 + 1.0e4 * (k % 97), nc.separators(n, [i for i in range(n) if (i + k0) % 3 != 1])


def wide_group(m, scaling):
    """one group of m producers under a limit on the total.  Progressive: the table's break falls on input 64 of 65, on input
    100 of 130 (the second 64 of the staging loop), in the middle otherwise"""
    rate, enth, sep = producers(m)
    b = {65: 64, 130: 100}.get(m, m // 2)
    limit = float(np.abs(rate[:b]).sum() + 0.5 * abs(rate[b]))
    spec = dict(rate_specified=[1] * m, enthalpy_specified=[0] * m, reinjectors=[],
                groups=[dict(inputs=[(1, i) for i in range(m)], scaling=scaling, limits=[(0, limit)], separator=None)])
    return nc.case(spec, rate, enth, sep)


def nested_wide(inner=70, outer_limit=20.0):
    """groups nested three deep around a wide inner group: a uniform group of `inner` producers with a steam limit, a
    progressive group between, a progressive total and water limit outside"""
    n = inner + 4
    rate, enth, sep = producers(n)
    spec = dict(rate_specified=[1] * n, enthalpy_specified=[0] * n, reinjectors=[], groups=[
        dict(inputs=[(1, i) for i in range(inner)], scaling=0, limits=[(2, 3.0)], separator=None),
        dict(inputs=[(1, inner), (2, 0), (1, inner + 1)], scaling=1, limits=[], separator=None),
        dict(inputs=[(1, inner + 2), (2, 1), (1, inner + 3)], scaling=1, limits=[(0, outer_limit), (1, 0.8 * outer_limit)], separator=None)])
    return nc.case(spec, rate, enth, sep)


def wide_reinjector(m=65):
    """three producers behind a group's separator feed a reinjector with m outputs (rate, proportion and unrated ones, water
    and steam, some with an enthalpy of their own, every fifth to nobody) and an overflow source"""
    n = 3 + m + 1
    rate = np.concatenate([[-6.0, -4.0, -5.0], 0.05 * (1 + np.arange(m) % 4), [0.0]])
    enth = np.concatenate([[1.3e6, 1.1e6, 1.6e6], np.full(m + 1, 3.0e5)])
    outs = []
    for i in range(m):
        mode = i % 3
        if mode == 2 and (i % 2 or i % 5 == 4):      # unrated only onto sources with a rate of their own: something is left
            mode = 0
        outs.append(dict(flow=1 + (i % 4 == 3), out=(0, -1) if i % 5 == 4 else (1, 3 + i), rate=0.02 * (1 + i % 7) if mode == 0 else -1.0,
                         proportion=0.01 * (1 + i % 5) if mode == 1 else -1.0, enthalpy=4.0e5 + 1.0e3 * i if i % 6 == 0 else -1.0))
    spec = dict(rate_specified=[1, 1, 1] + [int(i % 2 == 0) for i in range(m)] + [0], enthalpy_specified=[0] * 3 + [int(i % 7 == 0) for i in range(m)] + [0],
                groups=[dict(inputs=[(1, 0), (1, 1), (1, 2)], scaling=0, limits=[(0, 12.0)], separator=[(nc.HF, nc.HG)])],
                reinjectors=[dict(input=(2, 0), overflow=(1, n - 1), outputs=outs)])
    return nc.case(spec, rate, enth, nc.separators(n, []))


def two_outputs_one_source():
    """two outputs of one reinjector onto source 2, and the overflow of a second reinjector onto it as well: the last write
    wins, so the lanes must not deliver them side by side"""
    n = 5
    spec = dict(rate_specified=[1, 1, 0, 0, 0], enthalpy_specified=[0] * n,
                groups=[dict(inputs=[(1, 0), (1, 1)], scaling=0, limits=[], separator=[(nc.HF, nc.HG)])],
                reinjectors=[
                    dict(input=(2, 0), overflow=(3, 1), outputs=[
                        dict(flow=1, out=(1, 2), rate=0.7, proportion=-1.0, enthalpy=-1.0),
                        dict(flow=1, out=(1, 3), rate=-1.0, proportion=0.2, enthalpy=-1.0),
                        dict(flow=2, out=(1, 2), rate=-1.0, proportion=0.5, enthalpy=-1.0)]),
                    dict(input=(0, -1), overflow=(1, 2), outputs=[
                        dict(flow=1, out=(1, 4), rate=0.3, proportion=-1.0, enthalpy=-1.0)])])
    return nc.case(spec, [-6.0, -4.0, 0.0, 0.0, 0.0], [1.3e6, 1.1e6, 0.0, 0.0, 0.0])


def flat_behind_limit(n_prod, n_inj=2):
    """n_prod flat producers behind one limit, their water reinjected into n_inj sources, the rest to an overflow source"""
    n = n_prod + n_inj + 1
    rate, enth, sep = producers(n_prod)
    spec = dict(rate_specified=[1] * n_prod + [0] * (n_inj + 1), enthalpy_specified=[0] * n,
                groups=[dict(inputs=[(1, i) for i in range(n_prod)], scaling=0, limits=[(0, 0.3 * n_prod)], separator=None)],
                reinjectors=[dict(input=(2, 0), overflow=(1, n - 1), outputs=[
                    dict(flow=1, out=(1, n_prod + j), rate=-1.0, proportion=0.6 / n_inj, enthalpy=-1.0) for j in range(n_inj)])])
    return nc.case(spec, np.concatenate([rate, np.zeros(n_inj + 1)]), np.concatenate([enth, np.zeros(n_inj + 1)]),
                   np.concatenate([sep, np.zeros(8 * (n_inj + 1))]))


def source_in_two_groups():
    c = nc.three_wells(0)
    c["spec"]["groups"].append(dict(inputs=[(1, 1)], scaling=0, limits=[], separator=None))
    return c


def group_under_two_groups():
    c = nc.nested()
    c["spec"]["groups"].append(dict(inputs=[(2, 0)], scaling=0, limits=[], separator=None))
    return c


def wide_random(seed):
    """a seeded network of at most 200 sources, 6 groups and 4 reinjectors with fan-ins of up to 130: every source and group is
    taken in at most once; reinjectors deliver to injection sources (now and then to one that has a writer already), to later
    reinjectors or to nobody"""
    rng = np.random.default_rng(1000 + seed)
    n_prod, n_inj = int(rng.integers(20, 141)), int(rng.integers(5, 61))
    n = n_prod + n_inj
    rate = np.concatenate([-rng.uniform(0.0, 5.0, n_prod) * (rng.random(n_prod) > 0.1), rng.uniform(0.0, 3.0, n_inj) * (rng.random(n_inj) > 0.3)])
    enth = np.concatenate([rng.uniform(4.0e5, 3.0e6, n_prod), rng.uniform(8.0e4, 5.0e5, n_inj)])
    sep = np.zeros(8 * n)
    for i in range(n_prod):
        if rng.random() < 0.6:
            stages = [(nc.HF, nc.HG), (4.2e5, 2.68e6), (3.0e5, 2.6e6)][: int(rng.integers(1, 4))]
            sep[8 * i: 8 * i + 2 * len(stages)] = np.ravel(stages)
    free = [(1, i) for i in range(n_prod)]
    groups = []
    for g in range(int(rng.integers(1, 7))):
        if not free:
            break
        k = int(rng.integers(1, min(len(free), 130) + 1))
        if rng.random() < 0.35:
            k = min(k, 6)      # small groups keep nodes free for the nesting above them
        pick = [free.pop(int(rng.integers(0, len(free)))) for _ in range(k)]
        if groups and rng.random() < 0.6 and (2, g - 1) in free:      # nest the group before
            free.remove((2, g - 1))
            pick.insert(int(rng.integers(0, len(pick) + 1)), (2, g - 1))
        total = sum(abs(rate[i]) for kind, i in pick if kind == 1) + 1.0
        limits = [(int(rng.integers(0, 3)), float(rng.uniform(0.1, 1.2) * total)) for _ in range(int(rng.integers(0, 4)))]
        limits = list({t: (t, v) for t, v in limits}.values())
        groups.append(dict(inputs=pick, scaling=int(rng.integers(0, 2)), limits=limits,
                           separator=[(nc.HF, nc.HG)] if rng.random() < 0.4 else None))
        free.append((2, g))
    nr = int(rng.integers(0, 5))
    inj = list(range(n_prod, n))
    rng.shuffle(inj)
    used = []
    reinj = []
    for r in range(nr):
        outs = []
        for _ in range(int(rng.integers(0, 71))):
            u = rng.random()
            if u < 0.05 and used:
                out = (1, int(used[int(rng.integers(0, len(used)))]))      # a second writer
            elif u < 0.7 and inj:
                out = (1, int(inj.pop()))
                used.append(out[1])
            elif u < 0.8 and r + 1 < nr:
                out = (3, int(rng.integers(r + 1, nr)))
            else:
                out = (0, -1)
            mode = int(rng.integers(0, 3))
            outs.append(dict(flow=int(rng.integers(1, 3)), out=out, rate=float(rng.uniform(0.0, 0.5)) if mode == 0 else -1.0,
                             proportion=float(rng.uniform(0.0, 0.1)) if mode == 1 else -1.0,
                             enthalpy=float(rng.uniform(1.0e5, 5.0e5)) if rng.random() < 0.3 else -1.0))
        u = rng.random()
        if u < 0.3 and inj:
            over = (1, int(inj.pop()))
            used.append(over[1])
        elif u < 0.4 and used:
            over = (1, int(used[int(rng.integers(0, len(used)))]))
        else:
            over = (3, int(rng.integers(r + 1, nr))) if u < 0.7 and r + 1 < nr else (0, -1)
        src = free[int(rng.integers(0, len(free)))] if free and rng.random() < 0.8 else (0, -1)
        reinj.append(dict(input=src, overflow=over, outputs=outs))
    spec = dict(rate_specified=[int(rng.random() < 0.6) for _ in range(n)], enthalpy_specified=[int(rng.random() < 0.3) for _ in range(n)],
                groups=groups, reinjectors=reinj)
    return nc.case(spec, rate, enth, sep)


def schedule(spec):
    """the wave schedule from its definition: per group the sources below it (depth first, inputs in order), the groups below
    it (ascending), its ancestors (parent first), the positions among its inputs of those that are groups; per output whether its target source has another writer; the widest fan-in,
    the staging run and the doubles of LDS"""
    groups, reinj = spec["groups"], spec["reinjectors"]
    n, ng, nr = len(spec["rate_specified"]), len(groups), len(reinj)
    parent = {i: g for g, G in enumerate(groups) for k, i in G["inputs"] if k == 2}

    def sources_below(g):
        out = []
        for k, i in groups[g]["inputs"]:
            out += [i] if k == 1 else sources_below(i)
        return out

    def groups_below(g):
        out = set()
        for k, i in groups[g]["inputs"]:
            if k == 2:
                out |= {i} | set(groups_below(i))
        return sorted(out)

    def ancestors(g):
        out = []
        while g in parent:
            g = parent[g]
            out.append(g)
        return out

    def depth(g):
        return 1 + max([depth(i) for k, i in groups[g]["inputs"] if k == 2], default=0)

    def table(g):
        if not groups[g]["scaling"]:
            return 0
        return 3 * len(groups[g]["inputs"]) + max([table(i) for k, i in groups[g]["inputs"] if k == 2], default=0)

    def csr(lists):
        return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(int), np.array([y for x in lists for y in x], dtype=int)
    outs = [o for r in reinj for o in r["outputs"]]
    writers = {}
    for o in outs:
        if o["out"][0] == 1:
            writers[o["out"][1]] = writers.get(o["out"][1], 0) + 1
    for r in reinj:
        if r["overflow"][0] == 1:
            writers[r["overflow"][1]] = writers.get(r["overflow"][1], 0) + 1
    sch = {}
    sch["ds_ptr"], sch["ds"] = csr([sources_below(g) for g in range(ng)])
    sch["dg_ptr"], sch["dg"] = csr([groups_below(g) for g in range(ng)])
    sch["an_ptr"], sch["an"] = csr([ancestors(g) for g in range(ng)])
    sch["gc_ptr"], sch["gc"] = csr([[q for q, (k, i) in enumerate(G["inputs"]) if k == 2] for G in groups])
    sch["out_shared"] = np.array([int(o["out"][0] == 1 and writers[o["out"][1]] > 1) for o in outs], dtype=int)
    fan = max([len(G["inputs"]) for G in groups] + [len(r["outputs"]) for r in reinj] + [0])
    sch["fan_in"], sch["stage"] = np.array([fan]), np.array([CTL + STAGE * max(fan, 1)])
    # the lane walk's doubles (network_pass.hpp: description, raw rates, state) and what the wave walk adds
    n_in, n_out = sum(len(G["inputs"]) for G in groups), len(outs)
    n_iw = n + (ng + 1) + 5 * ng + 2 * n_in + 2 * nr + (nr + 1) + 3 * nr + 3 * n_out
    n_dw = 9 * n + 11 * ng + 3 * n_out
    frames = 2 * max([depth(g) for g in range(ng)], default=0) + 2
    arena = 3 + max([table(g) for g in range(ng)], default=0)
    state = 6 * (n + ng) + 15 * nr + 3 * n + arena + (4 * frames + 1) // 2
    n_ww = 4 * (ng + 1) + len(sch["ds"]) + len(sch["dg"]) + len(sch["an"]) + len(sch["gc"]) + n_out
    sch["lane_lds"] = n_dw + (n_iw + 1) // 2 + 2 * n + state
    sch["lds"] = np.array([sch["lane_lds"] + int(sch["stage"][0]) + (n_ww + 1) // 2])
    return sch
