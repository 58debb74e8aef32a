"""The symbolic phase of the tile-scheduled ILU sweeps without a GPU: csrc/tile_schedule.hpp (check_tiles: the refusals of
wai_set_pc_tiles; build_tile_schedule: tile levels, in-tile row levels, the sorted tile lists, `serve`) is pure host code; a
stand-alone program (tests/tile_schedule_host/main.cpp) built with the address and undefined-behaviour sanitizers calls it
behind build_host_schedule -- and behind build_asm_pattern for the extended systems -- and prints everything it makes.

Checked against a construction written here from the definitions (`TileTwin`): a tile is a run of consecutive rows of one
subdomain with one tile id; a tile's level is 0 without a predecessor tile, else 1 + the largest level among the tiles that
hold a coupled row; a row's in-tile level is the same recurrence over the couplings that stay in its tile; `serve` where the
tile levels of both sweeps are fewer than the row levels of both.  Slot ranges and row levels come from the Twin of
tests/test_pc_setup_host.py, the extended sets from tests/asm_reference.py (imported, not copied)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import asm_reference as ar
from tests import fused_reference as fr
from tests import wide_mesh
from tests.test_pc_setup_host import Twin, pattern
from waiwera_amd.cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = "big nlev_f nlev_b n_tiles ntl_f ntl_b max_tile_rows max_in_levels serve".split()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tile_schedule_host") / "tile_schedule_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tile_schedule_host", "main.cpp"), "-o", str(exe)])
    return str(exe)


def run(program, tmp_path, mode, **records):
    """what the program prints for the records: {"error": text} or {name: value(s)}; it exits 0 either way"""
    path = tmp_path / (mode + ".txt")
    with open(path, "w") as f:
        for name, v in records.items():
            v = np.atleast_1d(np.asarray(v, dtype=np.int64))
            f.write("%s %d %s\n" % (name, v.size, " ".join(map(str, v.tolist()))))
    p = subprocess.run([program, mode, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = {}
    for line in p.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "error":
            code, _, text = rest.partition(" ")
            return {"error": text, "code": int(code)}
        vals = np.array(rest.split(), dtype=np.int64)
        out[name] = int(vals[0]) if name in SCALARS else vals
    return out


def tiles(program, tmp_path, rp, ci, sub, tile_ptr, mode="tiles", **kw):
    return run(program, tmp_path, mode, rowptr=rp, colidx=ci, sub=sub, tile_ptr=tile_ptr, N=len(rp) - 1, W=int(np.diff(rp).max()),
               np=2, **kw)


class TileTwin:
    """tiles, tile levels and in-tile levels from the definitions, on the slot ranges and row levels of Twin"""

    def __init__(self, rp, ci, sub, row_tile):
        t = Twin(np.asarray(rp), np.asarray(ci), np.asarray(sub))
        n = t.n
        self.twin = t
        self.nlev_f, self.nlev_b = int(t.levf.max()) + 1, int(t.levb.max()) + 1
        row_tile = np.asarray(row_tile)
        start = np.ones(n, dtype=bool)
        start[1:] = (row_tile[1:] != row_tile[:-1]) | (t.brick[1:] != t.brick[:-1])
        self.tile_ptr = np.append(np.flatnonzero(start), n)
        self.tile = np.cumsum(start) - 1
        nt = len(self.tile_ptr) - 1
        self.lower = [sorted(k for k in t.inside[i] if k < i) for i in range(n)]
        self.upper = [sorted(k for k in t.inside[i] if k > i) for i in range(n)]
        tile = self.tile
        self.tlf, self.tlb = np.zeros(nt, dtype=np.int64), np.zeros(nt, dtype=np.int64)
        self.inf, self.inb = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for i in range(n):
            self.inf[i] = max([self.inf[k] + 1 for k in self.lower[i] if tile[k] == tile[i]], default=0)
        for i in reversed(range(n)):
            self.inb[i] = max([self.inb[k] + 1 for k in self.upper[i] if tile[k] == tile[i]], default=0)
        for T in range(nt):
            rows = range(self.tile_ptr[T], self.tile_ptr[T + 1])
            self.tlf[T] = max([self.tlf[tile[k]] + 1 for i in rows for k in self.lower[i] if tile[k] != T], default=0)
        for T in reversed(range(nt)):
            rows = range(self.tile_ptr[T], self.tile_ptr[T + 1])
            self.tlb[T] = max([self.tlb[tile[k]] + 1 for i in rows for k in self.upper[i] if tile[k] != T], default=0)
        self.ntl_f, self.ntl_b = int(self.tlf.max()) + 1, int(self.tlb.max()) + 1
        per = lambda v: np.array([v[a:b].max() + 1 for a, b in zip(self.tile_ptr[:-1], self.tile_ptr[1:])])
        self.ninf, self.ninb = per(self.inf), per(self.inb)
        self.serve = self.ntl_f + self.ntl_b < self.nlev_f + self.nlev_b


def check(out, tw):
    """everything the program printed against the twin, and the properties of the issue"""
    assert out["big"] == 1
    assert (out["nlev_f"], out["nlev_b"]) == (tw.nlev_f, tw.nlev_b)
    nt = len(tw.tile_ptr) - 1
    assert out["n_tiles"] == nt
    np.testing.assert_array_equal(out["tile_ptr"], tw.tile_ptr)
    np.testing.assert_array_equal(out["tile_lev"] & 0xffff, tw.tlf)
    np.testing.assert_array_equal(out["tile_lev"] >> 16, tw.tlb)
    np.testing.assert_array_equal(out["row_lev"] & 0xffff, tw.inf)
    np.testing.assert_array_equal(out["row_lev"] >> 16, tw.inb)
    np.testing.assert_array_equal(out["tile_nin"] & 0xffff, tw.ninf)
    np.testing.assert_array_equal(out["tile_nin"] >> 16, tw.ninb)
    assert (out["ntl_f"], out["ntl_b"]) == (tw.ntl_f, tw.ntl_b)
    assert out["max_tile_rows"] == np.diff(tw.tile_ptr).max() <= 1024
    assert out["max_in_levels"] == max(tw.ninf.max(), tw.ninb.max())
    assert out["serve"] == int(tw.serve)
    # every row belongs to exactly one tile: the ranges ascend strictly from 0 to n
    tp = out["tile_ptr"]
    assert tp[0] == 0 and tp[-1] == tw.twin.n and (np.diff(tp) > 0).all()
    # the sorted lists are permutations, each level's tiles are of that level, ascending
    for ordk, ptrk, lev, nl in (("ord_f", "tl_f_ptr", tw.tlf, tw.ntl_f), ("ord_b", "tl_b_ptr", tw.tlb, tw.ntl_b)):
        o, p = out[ordk], out[ptrk]
        np.testing.assert_array_equal(np.sort(o), np.arange(nt))
        assert len(p) == nl + 1 and p[0] == 0 and p[-1] == nt
        for l in range(nl):
            seg = o[p[l]:p[l + 1]]
            assert (lev[seg] == l).all() and (np.diff(seg) > 0).all()
    # on the program's own numbers: a coupled row of another tile lies at a strictly lower tile level, in-tile levels rise
    # strictly along in-tile couplings
    tile = tw.tile
    tlf, tlb = out["tile_lev"] & 0xffff, out["tile_lev"] >> 16
    inf, inb = out["row_lev"] & 0xffff, out["row_lev"] >> 16
    for i in range(tw.twin.n):
        for k in tw.lower[i]:
            assert tile[k] <= tile[i]
            assert (inf[k] < inf[i]) if tile[k] == tile[i] else (tlf[tile[k]] < tlf[tile[i]])
        for k in tw.upper[i]:
            assert tile[k] >= tile[i]
            assert (inb[k] < inb[i]) if tile[k] == tile[i] else (tlb[tile[k]] < tlb[tile[i]])


@functools.lru_cache(maxsize=None)
def box(dims, brick, **kw):
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos="we", **kw)
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64)


def ids(tile_ptr):
    return np.repeat(np.arange(len(tile_ptr) - 1), np.diff(tile_ptr))


TABLE = {   # the issue's table: (dims, bricks or None for 64-row ranges) -> tiles, tile levels, row levels, served
    "12x10x9": ((12, 10, 9), (4, 5, 3), 18, 6, 29, True),
    "13x10x9": ((13, 10, 9), (4, 5, 3), 24, 7, 30, True),
    "24x12x10": ((24, 12, 10), (8, 6, 5), 12, 5, 44, True),
    "chain": ((24, 12, 10), None, 45, 45, 44, False),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_table_of_level_counts(program, tmp_path, name):
    dims, brick, n_tiles, ntl, nlev, served = TABLE[name]
    rp, ci, bricks = box(dims, brick if brick else dims)
    n = len(rp) - 1
    tile_ptr = bricks if brick else np.append(np.arange(0, n, 64), n)
    sub = np.array([0, n])
    out = tiles(program, tmp_path, rp, ci, sub, tile_ptr)
    print(name, "tiles", out["n_tiles"], "tile levels", out["ntl_f"], out["ntl_b"], "row levels", out["nlev_f"], out["nlev_b"],
          "largest tile", out["max_tile_rows"], "in-tile depth", out["max_in_levels"], "serve", out["serve"])
    assert (out["n_tiles"], out["ntl_f"], out["ntl_b"], out["nlev_f"], out["nlev_b"], out["serve"]) == \
        (n_tiles, ntl, ntl, nlev, nlev, int(served))
    check(out, TileTwin(rp, ci, sub, ids(tile_ptr)))


def test_triangle_mesh(program, tmp_path):
    """a cell graph with triangles (off-diagonal fill in ILU(0)): 40 x 30 x 1 in one block, the 8 x 6 bricks its tiles"""
    g, lm, prim, region = fr.triangle_mesh(dims=(40, 30, 1), brick=(8, 6, 1))
    rp, ci = pattern(lm)
    n = len(rp) - 1
    sub, tile_ptr = np.array([0, n]), np.asarray(lm.sub_ptr, dtype=np.int64)
    assert n > 1024 and np.diff(rp).max() == 7      # one layer: 4 + 2 diagonals + itself
    out = tiles(program, tmp_path, rp, ci, sub, tile_ptr)
    check(out, TileTwin(rp, ci, sub, ids(tile_ptr)))
    assert out["serve"] == 1


def test_refined_wide_mesh(program, tmp_path):
    """rows of up to 16 blocks: the refined plan in enough layers for one block of more than 1024 rows, a tile per layer"""
    lm = wide_mesh.wide_case(layers=3)[0]
    nc = lm.n_owned // 3
    layers = 1024 // nc + 2
    lm = wide_mesh.wide_case(layers=layers)[0]
    rp, ci = pattern(lm)
    n = len(rp) - 1
    assert n == nc * layers > 1024 and np.diff(rp).max() > 8
    sub, tile_ptr = np.array([0, n]), np.arange(0, n + 1, nc)
    out = tiles(program, tmp_path, rp, ci, sub, tile_ptr)
    check(out, TileTwin(rp, ci, sub, ids(tile_ptr)))
    assert out["n_tiles"] == layers == out["ntl_f"] == out["ntl_b"]      # a chain of layers: served only if the rows' chain is longer
    assert out["serve"] == int(2 * layers < out["nlev_f"] + out["nlev_b"])


@functools.lru_cache(maxsize=None)
def two_slabs():
    """24 x 12 x 10 numbered in 6 x 6 x 5 bricks, x fastest: eight consecutive bricks are a 24 x 12 x 5 slab of 1440 rows"""
    rp, ci, bricks = box((24, 12, 10), (6, 6, 5), brick_order="x")
    assert len(bricks) == 17 and (np.diff(bricks) == 180).all()
    return rp, ci, np.array([0, 1440, 2880]), bricks


def test_two_subdomains_block_jacobi(program, tmp_path):
    rp, ci, sub, tile_ptr = two_slabs()
    out = tiles(program, tmp_path, rp, ci, sub, tile_ptr)
    tw = TileTwin(rp, ci, sub, ids(tile_ptr))
    check(out, tw)
    assert out["n_tiles"] == 16 and out["serve"] == 1
    # the slabs are independent and alike: the same levels in both
    np.testing.assert_array_equal(out["tile_lev"][:8], out["tile_lev"][8:])


@pytest.mark.parametrize("levels", [0, 1])
def test_two_subdomains_extended(program, tmp_path, levels):
    """PCASM overlap 1 (and with ILU(1) fill): the rows of E inherit the tiles of the rows they stand for -- contiguous inside
    a block, the neighbour slab's bricks with their overlap layer only"""
    rp, ci, sub, tile_ptr = two_slabs()
    out = tiles(program, tmp_path, rp, ci, sub, tile_ptr, mode="asm", overlap=1, levels=levels)
    ext_ptr, ext_row, owned = ar.extended_sets(rp, ci, sub, 1)
    np.testing.assert_array_equal(out["ext_ptr"], ext_ptr)
    np.testing.assert_array_equal(out["ext_rows"], ext_row)
    inherited = ids(tile_ptr)[ext_row]
    np.testing.assert_array_equal(out["etile"], inherited)
    tw = TileTwin(out["erp"], out["ecol"], ext_ptr, inherited)
    check(out, tw)
    # a block: its own 8 bricks whole and the 8 bricks of the other slab with one 6 x 6 layer each
    assert out["n_tiles"] == 32 and sorted(set(np.diff(out["tile_ptr"]).tolist())) == [36, 180]
    for b in range(2):
        run_ids = inherited[ext_ptr[b]:ext_ptr[b + 1]]
        assert (np.diff(run_ids) >= 0).all()      # contiguous: each inherited tile is one run
    assert out["serve"] == 1


def test_refusals(program, tmp_path):
    rp, ci, sub, tile_ptr = two_slabs()
    n = len(rp) - 1

    def text(tp, s=sub):
        out = tiles(program, tmp_path, rp, ci, s, np.asarray(tp))
        assert out.get("code") == -1, out
        return out["error"]
    assert text([0, 180, 170, n]) == "wai_set_pc_tiles: tile_ptr must ascend from 0 to n_owned (tile 1 ends before it starts)"
    assert text([4, 180, n]) == "wai_set_pc_tiles: tile_ptr must ascend from 0 to n_owned (tile 0 starts at row 4)"
    assert text(list(tile_ptr[:-1]) + [n - 1]) == "wai_set_pc_tiles: tile_ptr must ascend from 0 to n_owned (tile 15 ends at row 2879)"
    assert text(list(tile_ptr[:-1]) + [n + 1]) == "wai_set_pc_tiles: tile_ptr must ascend from 0 to n_owned (tile 15 ends at row 2881)"
    assert text([0, 180, 180] + list(tile_ptr[2:])) == "wai_set_pc_tiles: tile 1 is empty"
    assert text([0, 1025] + list(tile_ptr[6:])) == "wai_set_pc_tiles: tile 0 has 1025 rows, more than 1024"
    straddle = list(tile_ptr[:8]) + [1500] + list(tile_ptr[9:])
    assert text(straddle) == "wai_set_pc_tiles: tile 7 straddles a subdomain boundary (row 1440)"
    assert text([0]) == "wai_set_pc_tiles: tile_ptr must ascend from 0 to n_owned (no tile)"
    # the same list refines one block per rank
    assert "error" not in tiles(program, tmp_path, rp, ci, np.array([0, n]), np.asarray(straddle))
