"""The packing phase of csrc/ilu_schedule.hpp without a GPU: short bricks of a launch list share k_pc_park workgroups
(pack_groups).  A stand-alone program (tests/park_groups_host/main.cpp) built with the address and undefined-behaviour
sanitizers calls build_host_schedule on structured boxes in 16 x 16 x 2 bricks and prints the group tables; here they are
decoded record by record and held against the rules, and against a first-fit-decreasing twin written from the rules."""
import functools
import os
import subprocess

import numpy as np
import pytest

from waiwera_amd.cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(24, 24, 4), (20, 18, 5), (100, 100, 2), (216, 216, 2), (208, 208, 2)]
ORDERS = ["x", "tile4x4"]
LISTS = (0, 1, 2)            # all subdomains, interior bricks, face bricks


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("park_groups_host") / "park_groups_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "park_groups_host", "main.cpp"), "-o", str(exe)])
    return str(exe)


def pattern(lm):
    """(rowptr, colidx) of the owned cells' block rows: the cell itself and its neighbours among the owned and ghost cells"""
    n = lm.n_owned
    fc = np.asarray(lm.face_cells, dtype=np.int64)
    fc = fc[(fc < lm.n_prim).all(axis=1)]
    r = np.concatenate([np.arange(n), fc[:, 0], fc[:, 1]])
    c = np.concatenate([np.arange(n), fc[:, 1], fc[:, 0]])
    keep = r < n
    rc = np.unique(np.stack([r[keep], c[keep]], axis=1), axis=0)     # sorted by row, then column
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rc[:, 0], minlength=n))
    return rp, rc[:, 1]


@functools.lru_cache(maxsize=None)
def mesh(dims, order, part=(1, 1, 1)):
    g, lm, prim, region = make_case(dims=dims, brick=(16, 16, 2), eos="we", brick_order=order, order="hyperplane", part=part)
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), int(lm.n_halo)


@pytest.fixture(scope="module")
def built(program, tmp_path_factory):
    memo = {}

    def get(dims, order, part=(1, 1, 1)):
        key = (dims, order, part)
        if key not in memo:
            rp, ci, sub, n_halo = mesh(dims, order, part)
            W = int(np.diff(rp).max())
            rec = dict(rowptr=rp, colidx=ci, sub=sub, N=len(rp) - 1, W=W, np=2, ghosts=1, box_faces=int(n_halo == 0 and W == 7))
            path = tmp_path_factory.mktemp("case") / "in.txt"
            with open(path, "w") as f:
                for name, v in rec.items():
                    v = np.atleast_1d(np.asarray(v, dtype=np.int64))
                    f.write("%s %d %s\n" % (name, v.size, " ".join(map(str, v.tolist()))))
            p = subprocess.run([program, str(path)], capture_output=True, text=True)
            assert p.returncode == 0, p.stderr
            out = {}
            for line in p.stdout.splitlines():
                name, _, rest = line.partition(" ")
                out[name] = np.array(rest.split(), dtype=np.int64)
            memo[key] = out
        return memo[key]
    return get


def threads(rows):
    return (rows + 63) // 64 * 64


def members_of(s, which):
    """the table of list `which` decoded: per group (bricks in wave order, their thread offsets, park bases, level record);
    every record is checked against the rules on the way"""
    tab = s["groups%d" % which].reshape(-1, 8, 4)
    assert len(tab) == s["n_groups"][which]
    rows, max_ub = np.diff(s["sub"]), s["facts"][2]
    out = []
    for g in tab:
        bricks, offs, bases = [], [], []
        w = 0
        while w < 8:
            b, toff, ubase, nl = g[w]
            assert nl == g[0][3]                                   # one level record per group
            if b < 0:                                              # a wave without a brick
                w += 1
                continue
            nw = threads(rows[b]) // 64
            assert toff == 64 * w and toff % 64 == 0               # the member starts on this wave ...
            assert (g[w:w + nw, :3] == [b, toff, ubase]).all()      # ... and owns whole waves, as many as its rows need
            assert b not in bricks
            bricks.append(int(b)); offs.append(int(toff)); bases.append(int(ubase))
            w += nw
        assert 1 <= len(bricks) <= 8
        assert sum(threads(rows[b]) for b in bricks) <= 512         # (no overlap: the waves above are disjoint)
        uc = s["ucount"][bricks]
        assert uc.sum() <= max_ub and bases == (np.cumsum(uc) - uc).tolist()   # park ranges one behind the other, within the LDS request
        nlf, nlb = s["nlev"][bricks] & 0xffff, s["nlev"][bricks] >> 16
        assert g[0][3] == (nlf.max() | (nlb.max() << 16))          # the group's level counts: the maximum over its members
        out.append(bricks)
    return out


def ffd_twin(s, bricks):
    """first-fit decreasing over the short bricks of a list (ties by brick index); full bricks alone; a group at its first
    member's place; then per eighth the dear groups first (largest level counts, then rows), equal ones in their order"""
    rows, T, max_ub = np.diff(s["sub"]), threads(s["facts"][1]), s["facts"][2]
    bricks = sorted(bricks)
    bins = []
    for b in sorted((b for b in bricks if threads(rows[b]) < T), key=lambda b: (-rows[b], b)):
        for m in bins:
            if sum(threads(rows[x]) for x in m) + threads(rows[b]) <= T and s["ucount"][m].sum() + s["ucount"][b] <= max_ub:
                m.append(b)
                break
        else:
            bins.append([b])
    first = {m[0]: m for m in bins}
    groups = [first.get(b, [b]) for b in bricks if b in first or threads(rows[b]) >= T]

    def cost(m):
        return ((s["nlev"][m] & 0xffff).max() + (s["nlev"][m] >> 16).max()) * 4096 + rows[m].sum()
    per = (len(groups) + 7) // 8
    out = []
    for j in range(8):
        out += sorted(groups[j * per:(j + 1) * per], key=lambda m: -cost(m))     # (stable)
    return out, any(len(m) > 1 for m in bins)


def lists_of(s):
    nsub = s["facts"][0]
    return {0: list(range(nsub)), 1: s["sub_int"].tolist(), 2: s["sub_bnd"].tolist()}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dims", SHAPES)
def test_groups_follow_the_rules(built, dims, order):
    s = built(dims, order)
    assert s["facts"][3] == 1                                      # park_serves: the schedule the packing is for
    rows, info = np.diff(s["sub"]), s["info"]
    # the per-brick park counts: min(uppers, 3) per row, summed -- and their maximum is the launch's LDS request
    nu = np.minimum(((info >> 8) & 15) - ((info >> 4) & 15) - 1, 3)
    want = np.add.reduceat(nu, s["sub"][:-1])
    np.testing.assert_array_equal(s["ucount"], want)
    assert s["facts"][2] == want.max()
    for which, bricks in lists_of(s).items():
        twin, packs = ffd_twin(s, bricks) if bricks else ([], False)
        if not packs:                                              # nothing packs: no table, the launch of today
            assert s["n_groups"][which] == 0 and s["n_shared"][which] == 0 and s["groups%d" % which].size == 0
            continue
        got = members_of(s, which)
        assert sorted(b for m in got for b in m) == sorted(bricks)  # every brick of the list in exactly one group of it
        assert all(len(m) == 1 for m in got if threads(rows[m[0]]) == 512)        # full bricks stay alone
        assert got == twin
        assert s["n_shared"][which] == sum(len(m) for m in got if len(m) > 1)


@pytest.mark.parametrize("order", ORDERS)
def test_counts_of_the_benchmark_sizes(built, order):
    s = built((216, 216, 2), order)                                # a layer pair of C3: 169 full, 26 half and one quarter brick
    rows = np.diff(s["sub"])
    assert s["facts"][0] == 196 and sorted(np.unique(rows).tolist()) == [128, 256, 512]
    got = members_of(s, 0)
    assert len(got) == s["n_groups"][0] == 183 and s["n_shared"][0] == 26
    assert sorted(len(m) for m in got) == [1] * 170 + [2] * 13
    s = built((100, 100, 2), order)                                # a layer pair of C2: 36 full bricks, 12 of 128 rows, one of 32
    rows = np.diff(s["sub"])
    got = members_of(s, 0)
    assert len(got) == s["n_groups"][0] == 36 + 3 + 1 and s["n_shared"][0] == 12
    assert sorted(tuple(rows[m]) for m in got) == sorted([(512,)] * 36 + [(128,) * 4] * 3 + [(32,)])
    s = built((208, 208, 2), order)                                # nothing ragged: no tables
    assert (s["n_groups"] == 0).all() and all(s["groups%d" % k].size == 0 for k in LISTS)


@pytest.mark.parametrize("order", ORDERS)
def test_eight_bricks_can_share_a_workgroup(built, order):
    """20 x 18 x 5: members of 16, 64, 128 and 256 rows, idle waves"""
    s = built((20, 18, 5), order)
    rows = np.diff(s["sub"])
    assert {16, 64, 128, 256} <= set(rows.tolist())
    got = members_of(s, 0)
    assert any(sum(threads(rows[b]) for b in m) < 512 for m in got)          # some waves are idle


@pytest.mark.parametrize("order", ORDERS)
def test_interior_and_face_lists_pack_apart(built, order):
    """two ranks side by side, 24 x 24 x 4 each: the short bricks at the partition face are face bricks, those at the upper y
    end alone interior ones -- both lists have short bricks, and each packs its own"""
    s = built((48, 24, 4), order, part=(2, 1, 1))
    li, lb = s["sub_int"].tolist(), s["sub_bnd"].tolist()
    assert li and lb
    gi, gb = members_of(s, 1), members_of(s, 2)
    assert any(len(m) > 1 for m in gi) and any(len(m) > 1 for m in gb)
    assert sorted(b for m in gi for b in m) == sorted(li) and sorted(b for m in gb for b in m) == sorted(lb)
    assert gi == ffd_twin(s, li)[0] and gb == ffd_twin(s, lb)[0]
    # the list of all subdomains packs across both kinds -- its own table, used by the unsplit launch alone
    assert sorted(b for m in members_of(s, 0) for b in m) == sorted(li + lb)
