"""The symbolic phase of the two-level preconditioner's coarse space without a GPU: csrc/coarse_space.hpp (build_coarse_space)
is pure host code; a stand-alone program (tests/coarse_space_host/main.cpp) built with the address and undefined-behaviour
sanitizers calls it on small patterns and prints everything it makes.  Checked against a numpy construction written here
from the definition: an aggregate's rows are the cells i with agg[i] = I, ascending; coarse block (I, J) exists where some
block A_ij has i in I and j in J; its contributions are those (row, slot) pairs ordered by row, then slot."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.colour_reference import mesh_pattern as pattern
from tests import wide_mesh
from waiwera_amd.cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = "n nc bs max_rows".split()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("coarse_space_host") / "coarse_space_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "coarse_space_host", "main.cpp"), "-o", str(exe)])
    return str(exe)


def run(program, tmp_path, rp, ci, agg, nc, bs=2):
    path = tmp_path / "in.txt"
    with open(path, "w") as f:
        for name, v in dict(rowptr=rp, colidx=ci, agg=agg, N=len(rp) - 1, nc=nc, bs=bs).items():
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
        vals = np.array(rest.split(), dtype=np.int64)
        out[name] = int(vals[0]) if name in SCALARS else vals
    return out


def box(dims, brick):
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos="we")
    rp, ci = pattern(lm)
    return np.asarray(rp), np.asarray(ci), lm


def boxes_of(lm, dims, boxes):
    """aggregate of every owned cell: the mesh cut into boxes[a] boxes along axis a"""
    ijk = np.asarray(lm.owned_ijk)
    idx = [np.minimum(ijk[:, a] * boxes[a] // dims[a], boxes[a] - 1) for a in range(3)]
    return (idx[0] * boxes[1] + idx[1]) * boxes[2] + idx[2]


def case_442():
    rp, ci, lm = box((4, 4, 2), (2, 2, 2))
    return rp, ci, boxes_of(lm, (4, 4, 2), (2, 2, 1)), 4


def case_653():
    rp, ci, lm = box((6, 5, 3), (3, 5, 3))
    return rp, ci, boxes_of(lm, (6, 5, 3), (3, 2, 1)), 6


def case_one_cell():
    rp, ci, lm = box((6, 5, 3), (3, 5, 3))
    agg = boxes_of(lm, (6, 5, 3), (2, 1, 1))
    agg[37] = 2          # an aggregate of one cell, in the middle of another one
    return rp, ci, agg, 3


def case_all_in_one():
    rp, ci, lm = box((4, 4, 2), (2, 2, 2))
    return rp, ci, np.zeros(len(rp) - 1, dtype=np.int64), 1


def case_scrambled():
    rp, ci, lm = box((6, 5, 3), (3, 5, 3))
    rng = np.random.default_rng(7)
    agg = rng.integers(0, 11, len(rp) - 1)
    agg[:11] = rng.permutation(11)   # nobody empty
    return rp, ci, agg, 11


def case_wide():
    lm = wide_mesh.wide_case()[0]
    rp, ci = pattern(lm)
    n = len(rp) - 1
    assert int(np.diff(rp).max()) > 8
    return np.asarray(rp), np.asarray(ci), np.arange(n) * 5 // n, 5


CASES = {"4x4x2": case_442, "6x5x3": case_653, "one_cell": case_one_cell, "all_in_one": case_all_in_one,
         "scrambled": case_scrambled, "wide": case_wide}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def twin(rp, ci, agg, nc):
    """rows, pattern and lists from the definition"""
    n = len(rp) - 1
    rows = [np.nonzero(agg == I)[0] for I in range(nc)]
    blocks = {}
    for i in range(n):
        for s, j in enumerate(ci[rp[i]:rp[i + 1]]):
            if j < n:
                blocks.setdefault((int(agg[i]), int(agg[j])), []).append((i, s))
    return rows, {k: sorted(v) for k, v in blocks.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_coarse_space_against_the_definition(program, tmp_path, name):
    rp, ci, agg, nc = case(name)
    out = run(program, tmp_path, rp, ci, agg, nc)
    assert "error" not in out, out
    n = len(rp) - 1
    rows, blocks = twin(rp, ci, agg, nc)
    assert (out["n"], out["nc"], out["bs"]) == (n, nc, 2) and out["max_rows"] == max(len(r) for r in rows)
    assert np.array_equal(out["agg_ptr"], np.concatenate([[0], np.cumsum([len(r) for r in rows])]))
    assert np.array_equal(out["agg_rows"], np.concatenate(rows))
    # the coarse pattern: CSR over the aggregates, ascending columns, exactly the pairs the definition gives
    crp, cci, ep = out["c_rowptr"], out["c_colidx"], out["ent_ptr"]
    assert len(crp) == nc + 1 and crp[0] == 0 and crp[-1] == len(cci) == len(blocks) and len(ep) == len(cci) + 1
    pairs = [(I, int(J)) for I in range(nc) for J in cci[crp[I]:crp[I + 1]]]
    assert pairs == sorted(blocks)
    # every fine block of an owned column is in exactly one list, in (row, slot) order
    assert ep[0] == 0 and ep[-1] == len(out["ent_row"]) == len(out["ent_slot"]) == sum(len(v) for v in blocks.values())
    for b, key in enumerate(pairs):
        got = list(zip(out["ent_row"][ep[b]:ep[b + 1]].tolist(), out["ent_slot"][ep[b]:ep[b + 1]].tolist()))
        assert got == blocks[key], key


def test_one_cell_and_whole_mesh_aggregates(program, tmp_path):
    rp, ci, agg, nc = case("one_cell")
    out = run(program, tmp_path, rp, ci, agg, nc)
    assert out["agg_ptr"][3] - out["agg_ptr"][2] == 1 and out["agg_rows"][out["agg_ptr"][2]] == 37
    rp, ci, agg, nc = case("all_in_one")
    out = run(program, tmp_path, rp, ci, agg, nc)
    assert np.array_equal(out["c_rowptr"], [0, 1]) and np.array_equal(out["c_colidx"], [0]) and out["ent_ptr"][-1] == len(ci)
    assert out["max_rows"] == len(rp) - 1


def test_refusals(program, tmp_path):
    rp, ci, agg, nc = case("6x5x3")
    bad = agg.copy()
    bad[5] = nc
    msg = run(program, tmp_path, rp, ci, bad, nc)["error"]
    assert "agg[5] = %d is outside [0, nc = %d)" % (nc, nc) in msg, msg
    bad[5] = -1
    assert "agg[5] = -1 is outside" in run(program, tmp_path, rp, ci, bad, nc)["error"]
    msg = run(program, tmp_path, rp, ci, agg, nc + 1)["error"]
    assert "aggregate %d is empty" % nc in msg, msg
    # the cap counts unknowns: 513 aggregates of 2 x 2 blocks are 1026
    n = 600
    rp2, ci2 = np.arange(n + 1), np.arange(n)
    msg = run(program, tmp_path, rp2, ci2, np.arange(n) % 513, 513, bs=2)["error"]
    assert "nc * bs = 1026 coarse unknowns, more than 1024" in msg, msg
    assert "error" not in run(program, tmp_path, rp2, ci2, np.arange(n) % 512, 512, bs=2)
    assert "for each of the n_owned cells" in run(program, tmp_path, rp, ci, agg[:-1], nc)["error"]
