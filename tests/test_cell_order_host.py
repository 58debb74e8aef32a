"""The compact cell order without a GPU: csrc/cell_order.hpp (build_cell_order) is pure host code; a stand-alone program
(tests/cell_order_host/main.cpp) built with the address and undefined-behaviour sanitizers calls it on small meshes and
prints what it makes.  Checked for equality against the construction written in numpy from the definition
(tests/cell_order_cases.py: compact_order), and for the properties the preconditioner needs of it."""
import functools
import subprocess
import os

import numpy as np
import pytest

from tests import cell_order_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cell_order_host") / "cell_order_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cell_order_host", "main.cpp"), "-o", str(exe)])
    return str(exe)


def run(program, tmp_path, cen, faces, S):
    path = tmp_path / "in.txt"
    with open(path, "w") as f:
        f.write("n 1 %d\nS 1 %d\n" % (len(cen), S))
        flat = np.asarray(faces, dtype=np.int64).ravel()
        f.write("faces %d %s\n" % (flat.size, " ".join(map(str, flat.tolist()))))
        f.write("cen %d %s\n" % (3 * len(cen), " ".join(repr(float(v)) for v in np.asarray(cen).ravel())))
    p = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = {}
    for line in p.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "error":
            code, _, text = rest.partition(" ")
            assert int(code) == -2
            return {"error": text}
        out[name] = np.array(rest.split(), dtype=np.float64 if name == "h" else np.int64)
    out["n_sub"] = int(out["n_sub"][0])
    return out


def flat_mesh():
    """a 2-D mesh: one layer, so no face of the z axis (every face's largest centroid distance, 100, is horizontal) -- and z
    values whose extent in units of h = 1 is 50, four times that of x, which must not draw a split"""
    cen, faces = cc.hex_grid(13, 11, 1)
    cen[:, 2] = np.random.default_rng(5).uniform(0.0, 50.0, len(cen))
    return cen, faces, 16


def two_pieces():
    a, fa = cc.hex_grid(5, 4, 3)
    b, fb = cc.hex_grid(4, 6, 2)
    b[:, 0] += 5000.0
    return np.concatenate([a, b]), np.concatenate([fa, fb + len(a)]), 20


def scrambled(case):
    cen, faces, S = case()
    cs, fs, p = cc.scramble(cen, faces, 11)
    return cs, fs, S


CASES = {
    "hex_10x9x7": lambda: cc.hex_grid(10, 9, 7) + (100,),          # seven leaves; splits on several axes, ragged inside a plane
    "hex_24x20x6": lambda: cc.hex_grid(24, 20, 6) + (512,),
    "hex_32x32x8": lambda: cc.hex_grid(32, 32, 8) + (512,),
    "jittered_30x30x5": lambda: cc.hex_grid(30, 30, 5, jitter=0.3, seed=3) + (512,),    # all coordinates distinct
    "flat": flat_mesh,
    "column": lambda: cc.hex_grid(1, 1, 37) + (5,),
    "one_leaf": lambda: cc.hex_grid(4, 3, 2) + (24,),
    "one_leaf_roomy": lambda: cc.hex_grid(4, 3, 2) + (100,),
    "single_cells": lambda: cc.hex_grid(3, 3, 2) + (1,),
    "two_pieces": two_pieces,
    "no_faces": lambda: (np.random.default_rng(9).uniform(0.0, 1.0, (23, 3)), np.zeros((0, 2), dtype=np.int64), 4),
    "coincident": lambda: (np.zeros((9, 3)), np.zeros((0, 2), dtype=np.int64), 2),      # only the input index tells the cells apart
}
SCRAMBLED = ["hex_10x9x7", "hex_24x20x6", "hex_32x32x8", "jittered_30x30x5", "flat", "two_pieces"]
for _name in SCRAMBLED:
    CASES[_name + "_scrambled"] = functools.partial(scrambled, CASES[_name])
HEX = ["hex_10x9x7", "hex_24x20x6", "hex_32x32x8"]
GRIDS_3D = ["hex_24x20x6", "hex_32x32x8", "jittered_30x30x5"]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@pytest.fixture(scope="module")
def built(program, tmp_path_factory):
    memo = {}

    def get(name):
        if name not in memo:
            cen, faces, S = case(name)
            memo[name] = run(program, tmp_path_factory.mktemp(name), cen, faces, S)
        return memo[name]
    return get


@pytest.mark.parametrize("name", sorted(CASES))
def test_cell_order_against_the_definition(built, name):
    cen, faces, S = case(name)
    out = built(name)
    assert "error" not in out, out
    perm, sub = cc.compact_order(cen, faces, S)
    assert np.array_equal(out["h"], cc.spacings(cen, faces)[0])
    assert np.array_equal(out["sub_ptr"], sub) and out["n_sub"] == len(sub) - 1
    assert np.array_equal(out["perm"], perm)


@pytest.mark.parametrize("name", sorted(CASES))
def test_properties(built, program, tmp_path, name):
    cen, faces, S = case(name)
    out = built(name)
    n = len(cen)
    assert np.array_equal(np.sort(out["perm"]), np.arange(n))
    sub = out["sub_ptr"]
    assert sub[0] == 0 and sub[-1] == n and np.diff(sub).min() >= 1 and np.diff(sub).max() <= S
    assert out["n_sub"] <= -(-n // S)
    # the ordering of its own result is the identity
    c2, f2 = cc.renumbered(cen, faces, out["perm"])
    again = run(program, tmp_path, c2, f2, S)
    assert np.array_equal(again["perm"], np.arange(n)) and np.array_equal(again["sub_ptr"], sub)


def test_seven_leaves(built):
    assert built("hex_10x9x7")["n_sub"] == 7


def test_an_axis_without_faces_is_not_split_along(built):
    cen, faces, S = case("flat")
    out = built("flat")
    # every leaf of the 13 x 11 layer is a compact patch of it, whatever its z values are: were z split along, a leaf would
    # be scattered over the layer
    for s in range(out["n_sub"]):
        xy = cen[out["perm"][out["sub_ptr"][s]:out["sub_ptr"][s + 1]], :2]
        assert np.ptp(xy[:, 0]) * np.ptp(xy[:, 1]) <= 2 * S * 100.0 * 100.0, s


@pytest.mark.parametrize("name", SCRAMBLED)
def test_a_scrambled_file_gives_the_same_subdomains_in_the_same_order(built, name):
    cen, faces, S = case(name)
    p = cc.scramble(cen, faces, 11)[2]
    a, b = built(name), built(name + "_scrambled")
    assert np.array_equal(a["sub_ptr"], b["sub_ptr"])
    assert np.array_equal(p[b["perm"]], a["perm"])


@pytest.mark.parametrize("name", [g + s for g in GRIDS_3D for s in ("", "_scrambled")])
def test_cut_share_against_input_order_chunks(built, name):
    cen, faces, S = case(name)
    out = built(name)
    assert S == 512
    before = cc.cut_share(faces, cc.chunks(len(cen), S))
    after = cc.cut_share(cc.renumbered(cen, faces, out["perm"])[1], out["sub_ptr"])
    print("%s: interior faces cut %.3f in input-order chunks, %.3f in compact order" % (name, before, after))
    assert after < 0.5 * before


@pytest.mark.parametrize("name", [g + s for g in HEX + ["jittered_30x30x5"] for s in ("", "_scrambled")])
def test_coupling_counts(built, name):
    cen, faces, S = case(name)
    out = built(name)
    nl, nu = cc.coupling_counts(cc.renumbered(cen, faces, out["perm"])[1], out["sub_ptr"])
    print("%s: in-subdomain couplings lower %d upper %d; input-order chunks %s" % (name, nl, nu, cc.coupling_counts(faces, cc.chunks(len(cen), S))))
    if not name.startswith("jittered"):
        assert nl <= 3 and nu <= 3


def test_refusals(program, tmp_path):
    cen, faces, S = case("one_leaf")
    assert "cap must be at least 1" in run(program, tmp_path, cen, faces, 0)["error"]
    for bad in (len(cen), -1):
        f = faces.copy()
        f[3, 1] = bad
        assert "names a cell outside [0, n)" in run(program, tmp_path, cen, f, S)["error"]
    for bad in (np.nan, np.inf, -np.inf):
        c = cen.copy()
        c[5, 1] = bad
        assert "centroid is not finite" in run(program, tmp_path, c, faces, S)["error"]
