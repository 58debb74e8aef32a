"""The symbolic phase of the multicolour ILU(0) ordering without a GPU: csrc/colour_order.hpp (build_colour_order) is pure host
code; a stand-alone program (tests/colour_order_host/main.cpp) built with the address and undefined-behaviour sanitizers
calls it on small patterns and prints everything it makes.  Checked against a construction written here from the
definition: greedy colours per subdomain in ascending row index over the in-subdomain off-diagonal columns; elimination
order (colour, row index); a row's lower couplings are the in-subdomain columns eliminated before it."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import fused_reference as fr
from tests.colour_reference import mesh_pattern as pattern
from tests import wide_mesh
from waiwera_amd.cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = "nsub max_rows max_colours diag_only max_blocks".split()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("colour_order_host") / "colour_order_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "colour_order_host", "main.cpp"), "-o", str(exe)])
    return str(exe)


def run(program, tmp_path, rp, ci, sub):
    path = tmp_path / "in.txt"
    with open(path, "w") as f:
        for name, v in dict(rowptr=rp, colidx=ci, sub=sub, N=len(rp) - 1).items():
            v = np.atleast_1d(np.asarray(v, dtype=np.int64))
            f.write("%s %d %s\n" % (name, v.size, " ".join(map(str, v.tolist()))))
    p = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = {}
    for line in p.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "error":
            code, _, text = rest.partition(" ")
            assert int(code) == -2
            return {"error": text}
        vals = np.array(rest.split(), dtype=np.uint64 if name == "slots" else np.int64)
        out[name] = int(vals[0]) if name in SCALARS else vals
    return out


def box(dims, brick, **kw):
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos="we", **kw)
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), lm


def one_block():
    rp, ci, sub, lm = box((7, 5, 3), (4, 3, 2))
    return rp, ci, np.array([0, len(rp) - 1]), lm


def triangle():
    g, lm, prim, region = fr.triangle_mesh()
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), lm


def wide():
    lm = wide_mesh.wide_case()[0]
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), lm


CASES = {
    "bricks_hyperplane": lambda: box((6, 6, 4), (3, 3, 2)),
    "bricks_natural": lambda: box((6, 6, 4), (3, 3, 2), order="natural"),
    "ragged": lambda: box((7, 5, 3), (4, 3, 2)),
    "one_block": one_block,
    "two_ranks": lambda: box((8, 6, 4), (4, 3, 2), part=(2, 1, 1)),   # ghost columns >= n are nobody's neighbours
    "minc": lambda: box((6, 4, 2), (3, 2, 2), minc=True),
    "triangle": triangle,
    "wide": wide,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@pytest.fixture(scope="module")
def built(program, tmp_path_factory):
    memo = {}

    def get(name):
        if name not in memo:
            rp, ci, sub, lm = case(name)
            memo[name] = run(program, tmp_path_factory.mktemp(name), rp, ci, sub)
        return memo[name]
    return get


class Twin:
    """colours, elimination order and descriptors from the definition"""

    def __init__(self, rp, ci, sub):
        n = len(rp) - 1
        self.n = n
        owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
        self.nbr = []          # per row: [(column, slot)] of the in-subdomain off-diagonal blocks
        self.dslot = np.zeros(n, dtype=np.int64)
        for i in range(n):
            cols = ci[rp[i]:rp[i + 1]]
            self.dslot[i] = int(np.nonzero(cols == i)[0][0])
            self.nbr.append([(int(j), q) for q, j in enumerate(cols) if j != i and j < n and owner[j] == owner[i]])
        self.colour = np.full(n, -1, dtype=np.int64)
        for i in range(n):
            taken = {self.colour[j] for j, _ in self.nbr[i] if j < i}
            c = 0
            while c in taken:
                c += 1
            self.colour[i] = c
        self.ncolours = np.array([self.colour[sub[s]:sub[s + 1]].max() + 1 if sub[s + 1] > sub[s] else 0 for s in range(len(sub) - 1)])
        key = self.colour * n + np.arange(n)
        self.lower = [[q for j, q in sorted(self.nbr[i], key=lambda e: key[e[0]]) if key[j] < key[i]] for i in range(n)]
        self.upper = [[q for j, q in sorted(self.nbr[i], key=lambda e: key[e[0]]) if key[j] > key[i]] for i in range(n)]
        # the graph's triangles inside a subdomain
        sets = [{j for j, _ in nb} for nb in self.nbr]
        self.triangles = any(sets[i] & sets[j] for i in range(n) for j in sets[i])


@pytest.mark.parametrize("name", sorted(CASES))
def test_colour_order_against_the_definition(built, name):
    rp, ci, sub, lm = case(name)
    out = built(name)
    assert "error" not in out, out
    t = Twin(rp, ci, sub)
    n = t.n
    assert out["nsub"] == len(sub) - 1 and out["max_rows"] == int(np.diff(sub).max()) and np.array_equal(out["sub"], sub)
    assert out["max_blocks"] == int(np.diff(rp).max())
    # no two coupled rows of a subdomain share a colour; the colours are the greedy ones
    for i in range(n):
        for j, _ in t.nbr[i]:
            assert out["colour"][i] != out["colour"][j], (i, j)
    assert np.array_equal(out["colour"], t.colour)
    assert np.array_equal(out["ncolours"], t.ncolours) and out["max_colours"] == int(t.ncolours.max())
    assert out["diag_only"] == (0 if t.triangles else 1)
    # the descriptors: lower and upper sets and their order, the diagonal slot
    for i in range(n):
        cnt, pack = int(out["counts"][i]), int(out["slots"][i])
        nl, nu, ds = cnt & 0xff, (cnt >> 8) & 0xff, (cnt >> 16) & 0xff
        slots = [(pack >> (4 * p)) & 15 for p in range(nl + nu)]
        assert ds == t.dslot[i] and cnt >> 24 == t.colour[i], i
        assert slots[:nl] == t.lower[i] and slots[nl:] == t.upper[i], (i, slots, t.lower[i], t.upper[i])
        assert pack >> (4 * (nl + nu)) == 0
    # the launch lists partition the rows: colour c's range holds exactly the rows of colour c, ascending
    cp = out["col_ptr"]
    assert len(cp) == out["max_colours"] + 1 and cp[0] == 0 and cp[-1] == n
    assert np.array_equal(np.sort(out["rows"]), np.arange(n))
    for c in range(out["max_colours"]):
        assert np.array_equal(out["rows"][cp[c]:cp[c + 1]], np.nonzero(t.colour == c)[0])


@pytest.mark.parametrize("name", ["bricks_hyperplane", "bricks_natural", "ragged", "one_block"])
def test_box_meshes_have_two_colours_by_parity(built, name):
    rp, ci, sub, lm = case(name)
    out = built(name)
    assert out["max_colours"] == 2 and out["diag_only"] == 1 and set(out["ncolours"].tolist()) == {2}
    ijk = np.asarray(lm.owned_ijk)
    for s in range(len(sub) - 1):
        rows = np.arange(sub[s], sub[s + 1])
        rel = ijk[rows] - ijk[rows].min(axis=0)
        assert np.array_equal(out["colour"][rows], rel.sum(axis=1) % 2), s


def test_minc_has_two_colours(built):
    out = built("minc")
    assert out["max_colours"] == 2 and out["diag_only"] == 1


def test_triangles_need_three_colours_and_a_stored_factor(built):
    out = built("triangle")
    assert out["max_colours"] >= 3 and out["diag_only"] == 0


def test_wide_rows(built):
    out = built("wide")
    assert out["max_blocks"] == 15 and 2 <= out["max_colours"] <= 16


def test_refusals(program, tmp_path):
    rp, ci, sub, lm = case("ragged")
    assert "sub_ptr must cover" in run(program, tmp_path, rp, ci, sub[:-1])["error"]
    # a row of 17 blocks
    n = 18
    rows = [list(range(17))] + [[0, i] for i in range(1, 17)] + [[17]]
    rp2 = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    assert "more than 16 blocks" in run(program, tmp_path, rp2, np.concatenate(rows), np.array([0, n]))["error"]
    # row 0 has column 1, row 1 has no column 0: both get colour 0
    rows = [[0, 1], [1]]
    assert "structurally symmetric" in run(program, tmp_path, np.array([0, 2, 3]), np.concatenate(rows), np.array([0, 2]))["error"]
