"""The symbolic phase of the preconditioner without a GPU: csrc/ilu_schedule.hpp (build_host_schedule: every fact and table
of an IluSchedule) and csrc/asm_pattern.hpp (build_asm_pattern: the extended system of PCASM / ILU(k) / sub-preconditioner
lu) are pure host code; a stand-alone program (tests/pc_setup_host/main.cpp) built with the address and undefined-behaviour
sanitizers calls them on small patterns and prints everything they make.

The schedule is checked against constructions written here from the definitions (`Twin`: slot ranges from the sorted
columns and the subdomain's range, levels from the recurrence, a direct symbolic ILU(0) for diag_only), its packed tables
are decoded field by field, and the 16-bit indices and the shared descriptors are checked as properties.  The extended
pattern is checked against the twins the GPU tests already use: extended_sets / extended_pattern of tests/asm_reference.py
and iluk_pattern of tests/test_hip_iluk_fused.py (imported, not copied)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import asm_reference as ar
from tests import fused_reference as fr
from tests import wide_mesh
from tests.test_hip_iluk_fused import iluk_pattern
from waiwera_amd.cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ("nsub max_rows max_lev max_nl max_nlu max_ublocks max_ublocks_w n_int n_bnd nlev_f nlev_b n_templates template_rows "
           "wide big sublu diag_only scaled park fast3 rows_kernel wave_kernel park_serves W").split()
OPTS = dict(ghosts=1, allow_wide=1, sublu=0, fill=0, box_faces=0, max_seg=8, ilu_general=0, pc_rows=-1, pc_wave=1)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pc_setup_host") / "pc_setup_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pc_setup_host", "main.cpp"), "-o", str(exe)])
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
            assert int(code) == -2
            return {"error": text}
        vals = np.array(rest.split(), dtype=np.int64)
        out[name] = int(vals[0]) if name in SCALARS else vals
    return out


def schedule(program, tmp_path, rp, ci, sub, np_, **opts):
    W = int(np.diff(rp).max())
    o = dict(OPTS, mesh_W=W)
    o.update(opts)
    return run(program, tmp_path, "schedule", rowptr=rp, colidx=ci, sub=sub, N=len(rp) - 1, W=W, np=np_, **o)


def pattern(lm):
    """(rowptr, colidx) of the owned cells' block rows: the cell itself and its neighbours among the owned and ghost cells"""
    n = lm.n_owned
    nb = [{i} for i in range(n)]
    for a, b in np.asarray(lm.face_cells).tolist():
        if a < n and b < lm.n_prim:
            nb[a].add(b)
        if b < n and a < lm.n_prim:
            nb[b].add(a)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(s) for s in nb])
    return rp, np.array([j for s in nb for j in sorted(s)], dtype=np.int64)


# ---- the schedule's cases: name -> (rowptr, colidx, sub, block size, options) -------------------------------------------
def box(dims, brick, np_, **kw):
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos={2: "we", 3: "wce", 4: "wsce"}[np_], **kw)
    rp, ci = pattern(lm)
    # (what the library does on one rank: a 7-point mesh's box faces stand for partition boundaries)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), np_, dict(box_faces=int(lm.n_halo == 0 and np.diff(rp).max() == 7))


def triangle():
    g, lm, prim, region = fr.triangle_mesh()
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), 2, {}


def wide():
    lm = wide_mesh.wide_case()[0]
    rp, ci = pattern(lm)
    return rp, ci, np.asarray(lm.sub_ptr, dtype=np.int64), 2, {}


def asymmetric():
    """six rows in two subdomains; row 1 has column 0 and row 0 no column 1 (tslot 15), row 2 reaches the other subdomain"""
    rows = [[0, 2], [0, 1, 2], [0, 1, 2, 4], [3, 5], [2, 3, 4], [4, 5]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return rp, np.concatenate(rows), np.array([0, 3, 6]), 2, {}


SMALL = {
    "ragged": lambda: box((12, 10, 9), (4, 4, 2), 2),            # ragged bricks: an order exists; col16 and templates
    "wave": lambda: box((13, 9, 5), (5, 4, 2), 3),               # the wave kernel; one interior brick
    "minc_split": lambda: box((16, 8, 4), (4, 4, 1), 3, minc=True),   # the split record with short rows
    "minc_nlu4": lambda: box((8, 8, 4), (4, 4, 4), 3, minc=True),     # max_nlu == 4, the rows kernel
    "rows": lambda: box((8, 8, 4), (4, 2, 2), 4),                # the rows kernel
    "big": lambda: box((16, 16, 10), (16, 16, 5), 2),            # 1280 rows in a subdomain: level sets
    "two_ranks": lambda: box((16, 8, 4), (4, 4, 2), 2, part=(2, 1, 1)),   # ghost columns: interior and face bricks
    "triangle": triangle,                                        # off-diagonal fill
    "wide": wide,                                                # rows of more than 8 blocks: the 64-bit descriptor
    "asymmetric": asymmetric,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return SMALL[name]()


@pytest.fixture(scope="module")
def built(program, tmp_path_factory):
    """name -> the program's output for the case, built once"""
    memo = {}

    def get(name):
        if name not in memo:
            rp, ci, sub, np_, opts = case(name)
            memo[name] = schedule(program, tmp_path_factory.mktemp(name), rp, ci, sub, np_, **opts)
        return memo[name]
    return get


class Twin:
    """slot ranges, levels and what follows from them, from the definitions"""

    def __init__(self, rp, ci, sub):
        n = len(rp) - 1
        self.n, self.sub = n, sub
        self.brick = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
        self.cols = [ci[rp[i]:rp[i + 1]] for i in range(n)]
        lo, hi = sub[self.brick], sub[self.brick + 1]
        # slots [lfirst, ulast) of a row hold the columns inside its subdomain, slot dslot the diagonal
        self.lfirst = np.array([(c < a).sum() for c, a in zip(self.cols, lo)])
        self.ulast = np.array([(c < b).sum() for c, b in zip(self.cols, hi)])
        self.dslot = np.array([(c < i).sum() for i, c in enumerate(self.cols)])
        self.inside = [set(c[(c >= a) & (c < b)].tolist()) for c, a, b in zip(self.cols, lo, hi)]
        self.levf, self.levb = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for i in range(n):
            self.levf[i] = max([self.levf[k] + 1 for k in self.inside[i] if k < i], default=0)
        for i in reversed(range(n)):
            self.levb[i] = max([self.levb[k] + 1 for k in self.inside[i] if k > i], default=0)
        self.lower = self.dslot - self.lfirst
        self.upper = self.ulast - self.dslot - 1

    def per_brick(self, v, f):
        return np.array([f(v[a:b]) for a, b in zip(self.sub[:-1], self.sub[1:])])

    def elimination_updates_an_offdiagonal_block(self):
        """symbolic ILU(0), IKJ: row k < i of the subdomain eliminated from row i updates A_ij for the j > k that both rows have"""
        for i in range(self.n):
            for k in self.inside[i]:
                if k < i and any(j > k and j != i and j in self.inside[i] for j in self.inside[k]):
                    return True
        return False

    def cost(self):
        return (self.per_brick(self.levf, max) + 1 + self.per_brick(self.levb, max) + 1) * 4096 + np.diff(self.sub)


@functools.lru_cache(maxsize=None)
def twin(name):
    rp, ci, sub, np_, opts = case(name)
    return Twin(rp, ci, sub)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_slot_ranges_levels_and_descriptors(built, name):
    s, t = built(name), twin(name)
    nlf, nlb = t.per_brick(t.levf, max) + 1, t.per_brick(t.levb, max) + 1
    np.testing.assert_array_equal(s["nlev"] & 0xffff, nlf)
    np.testing.assert_array_equal(s["nlev"] >> 16, nlb)
    np.testing.assert_array_equal(s["sub"], t.sub)
    info = s["info"]
    if s["big"] or s["wide"]:       # 8-bit slots, no levels
        fields = (info & 255, (info >> 8) & 255, info >> 16)
    else:                           # 4-bit slots, 10-bit levels
        fields = (info & 15, (info >> 4) & 15, (info >> 8) & 15)
        np.testing.assert_array_equal((info >> 12) & 1023, t.levf)
        np.testing.assert_array_equal((info & 0xffffffff) >> 22, t.levb)
    for got, want in zip(fields, (t.lfirst, t.dslot, t.ulast)):
        np.testing.assert_array_equal(got, want)
    if s["wide"]:                   # the 64-bit descriptor: 5-bit slots in the low word, 10-bit levels in the high one
        w = s["infow"]
        for got, want in zip((w & 31, (w >> 5) & 31, (w >> 10) & 31, (w >> 32) & 1023, w >> 42),
                             (t.lfirst, t.dslot, t.ulast, t.levf, t.levb)):
            np.testing.assert_array_equal(got, want)
    else:
        assert s["infow"].size == 0


@pytest.mark.parametrize("name", sorted(SMALL))
def test_offsets_slots_and_extremes(built, name):
    s, t = built(name), twin(name)
    start = np.repeat(t.sub[:-1], np.diff(t.sub))
    for key, counted in (("uoff", np.minimum(t.upper, 3)), ("uoffw", t.upper)):
        run_sum = np.cumsum(counted) - counted
        np.testing.assert_array_equal(s[key], run_sum - run_sum[start], err_msg=key)
    for i in range(t.n):             # nibble p: the slot of row k (the p-th lower coupling of row i) that holds column i
        low = sorted(k for k in t.inside[i] if k < i)[:4]
        for p in range(8):
            slot = (s["tslot"][i] >> (4 * p)) & 15
            if p >= len(low):
                assert slot == 0
            elif i in t.cols[low[p]]:
                assert t.cols[low[p]][slot] == i
            else:
                assert slot == 15
    assert s["max_rows"] == np.diff(t.sub).max() and s["nsub"] == len(t.sub) - 1
    assert s["max_lev"] == max(t.levf.max(), t.levb.max()) + 1
    assert s["max_nl"] == t.lower.max() and s["max_nlu"] == max(t.lower.max(), t.upper.max())
    assert s["max_ublocks"] == t.per_brick(np.minimum(t.upper, 3), sum).max()
    assert s["max_ublocks_w"] == t.per_brick(t.upper, sum).max()
    assert s["fast3"] == int(t.lower.max() <= 3 and t.upper.max() <= 3 and t.lfirst.max() <= 3 and t.dslot.max() <= 3)
    assert s["diag_only"] == int(not t.elimination_updates_an_offdiagonal_block() and not s["big"] and not s["wide"])


@pytest.mark.parametrize("name", sorted(SMALL))
def test_launch_order(built, name):
    s, t = built(name), twin(name)
    cost, order, nsub = t.cost(), s["order"], len(t.sub) - 1
    if s["big"] or (cost == cost[0]).all():
        assert order.size == 0
        return
    assert sorted(order.tolist()) == list(range(nsub))
    per = (nsub + 7) // 8
    for j in range(8):               # each eighth keeps its bricks; the dear ones first, equal ones in their order
        part = order[j * per:(j + 1) * per].tolist()
        assert sorted(part) == list(range(min(j * per, nsub), min((j + 1) * per, nsub)))
        assert part == sorted(part, key=lambda b: (-cost[b], b))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_interior_and_face_lists(built, name):
    s, t = built(name), twin(name)
    rp, ci, sub, np_, opts = case(name)
    if opts.get("box_faces"):
        face = t.per_brick(np.diff(rp) < 7, any)
    else:
        face = t.per_brick(np.array([c.max() >= t.n for c in t.cols]), any)
    assert (s["n_int"], s["n_bnd"]) == ((~face).sum(), face.sum())
    if face.all() or not face.any():
        assert s["sub_int"].size == 0 and s["sub_bnd"].size == 0
    else:
        assert sorted(s["sub_int"].tolist()) == np.flatnonzero(~face).tolist()
        assert sorted(s["sub_bnd"].tolist()) == np.flatnonzero(face).tolist()


@pytest.mark.parametrize("name", sorted(SMALL))
def test_level_sets(built, name):
    s, t = built(name), twin(name)
    if not (s["big"] or s["wide"]):
        assert s["ord_f"].size == 0 and s["ord_b"].size == 0 and s["lev_f_ptr"].size == 0 and s["nlev_f"] == 0
        return
    for lev, ptr, order, nlev in ((t.levf, s["lev_f_ptr"], s["ord_f"], s["nlev_f"]), (t.levb, s["lev_b_ptr"], s["ord_b"], s["nlev_b"])):
        assert nlev == lev.max() + 1 and len(ptr) == nlev + 1 and ptr[0] == 0 and ptr[-1] == t.n
        for l in range(nlev):
            np.testing.assert_array_equal(order[ptr[l]:ptr[l + 1]], np.flatnonzero(lev == l))


def test_sub_lu_schedule_has_no_level_sets(program, tmp_path):
    rp, ci, sub, np_, opts = case("rows")
    s = schedule(program, tmp_path, rp, ci, sub, np_, ghosts=0, sublu=1)
    assert s["big"] and s["sublu"] and not s["wide"] and s["ord_f"].size == 0 and s["lev_f_ptr"].size == 0 and s["nlev_f"] == 0
    np.testing.assert_array_equal(s["info"] & 255, twin("rows").lfirst)


@pytest.mark.parametrize("name", ["minc_split", "minc_nlu4", "rows"])
def test_split_record(built, name):
    """low half: the leading rows of more than W / 2 blocks where they come first and no such row follows, else all rows;
    high half: the most blocks of a row behind them, or 15 where a long row follows a short one.  The table exists where
    some brick is split"""
    s, t = built(name), twin(name)
    rp = case(name)[0]
    W = np.diff(rp).max()
    want = []
    for a, b in zip(t.sub[:-1], t.sub[1:]):
        cnt = np.diff(rp)[a:b]
        long_ = cnt * 2 > W
        lead = len(long_) if long_.all() else int(np.argmin(long_))
        clean = not long_[lead:].any()
        rows = lead if clean and lead > 0 else b - a
        want.append(rows | ((max(cnt[lead:], default=0) if clean else 15) << 16))
    want = np.array(want)
    assert s["rows_kernel"]
    if ((want & 0xffff) != np.diff(t.sub)).any():
        np.testing.assert_array_equal(s["split"], want)
    else:
        assert s["split"].size == 0


def check_col16(s, rp, ci, sub):
    """for every row and slot, sub_seg[brick][c >> 13] + (c & 8191) is the block-ELL column (padding: the row itself)"""
    n, W = len(rp) - 1, int(np.diff(rp).max())
    c16, seg = s["c16"].reshape(n, 8), s["seg"].reshape(-1, 8)
    brick = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
    ell = np.tile(np.arange(n)[:, None], (1, W))
    slot = np.arange(rp[-1]) - np.repeat(rp[:-1], np.diff(rp))
    ell[np.repeat(np.arange(n), np.diff(rp)), slot] = ci
    np.testing.assert_array_equal(seg[brick[:, None], c16[:, :W] >> 13] + (c16[:, :W] & 8191), ell)
    np.testing.assert_array_equal(seg[:, 0], sub[:-1])
    assert (c16[:, W:] == 0).all()


def check_templates(s, sub):
    """rows [desc[b], desc[b] + rows of b) of the template tables are brick b's own rows byte for byte; as many templates as
    there are distinct (row count, info, uoff, c16) byte strings"""
    info, uoff, c16 = s["info"].astype(np.int32), s["uoff"].astype(np.int32), s["c16"].astype(np.uint16).reshape(-1, 8)
    ti, tu, tc = s["t_info"].astype(np.int32), s["t_uoff"].astype(np.int32), s["t_c16"].astype(np.uint16).reshape(-1, 8)
    distinct = set()
    for b, (lo, hi) in enumerate(zip(sub[:-1], sub[1:])):
        d, R = s["desc"][b], hi - lo
        assert ti[d:d + R].tobytes() == info[lo:hi].tobytes() and tu[d:d + R].tobytes() == uoff[lo:hi].tobytes()
        assert tc[d:d + R].tobytes() == c16[lo:hi].tobytes()
        distinct.add((R, info[lo:hi].tobytes(), uoff[lo:hi].tobytes(), c16[lo:hi].tobytes()))
    assert s["n_templates"] == len(distinct)
    assert s["template_rows"] == len(ti) == sum(k[0] for k in distinct)


@pytest.mark.parametrize("name", ["ragged", "two_ranks"])
def test_col16_and_templates_small(built, name):
    s = built(name)
    rp, ci, sub, np_, opts = case(name)
    assert s["park_serves"]
    check_col16(s, rp, ci, sub)
    check_templates(s, sub)


@pytest.mark.parametrize("dims, templates, bricks", [((48, 48, 4), 18, 18), ((64, 64, 6), 27, 48)])
def test_template_counts_of_the_structured_boxes(program, tmp_path, dims, templates, bricks):
    """the counts tests/test_hip_park_descriptors.py asserts on the device"""
    rp, ci, sub, np_, opts = box(dims, (16, 16, 2), 2, lens=True, brick_order="x", order="hyperplane")
    s = schedule(program, tmp_path, rp, ci, sub, np_, **opts)
    assert (s["n_templates"], s["nsub"], s["template_rows"]) == (templates, bricks, 512 * templates)
    check_col16(s, rp, ci, sub)
    check_templates(s, sub)
    if dims == (48, 48, 4):          # the same mesh with one segment allowed: no 16-bit indices, nothing shared
        s = schedule(program, tmp_path, rp, ci, sub, np_, **dict(opts, max_seg=1))
        assert s["park_serves"] and s["n_templates"] == 0 and s["template_rows"] == 0
        assert all(s[k].size == 0 for k in ("c16", "seg", "t_info", "t_uoff", "t_c16", "desc"))


def test_the_cases_reach_the_branches_they_are_for(built):
    flags = ("big", "wide", "diag_only", "park_serves", "rows_kernel", "wave_kernel")
    want = {"ragged": (0, 0, 1, 1, 0, 0), "wave": (0, 0, 1, 0, 1, 1), "minc_split": (0, 0, 1, 0, 1, 1), "minc_nlu4": (0, 0, 1, 0, 1, 0),
            "rows": (0, 0, 1, 0, 1, 0), "big": (1, 0, 0, 0, 0, 0), "two_ranks": (0, 0, 1, 1, 0, 0), "triangle": (0, 0, 0, 0, 0, 0),
            "wide": (0, 1, 0, 0, 0, 0), "asymmetric": (0, 0, 0, 0, 0, 0)}
    for name in sorted(SMALL):
        s = built(name)
        assert tuple(s[f] for f in flags) == want[name], name
        # parked upper blocks: the solution entries of whole waves, 32 doubles of scratch and four doubles per parked block in 64 KB
        lds = ((s["max_rows"] + 63) // 64 * 64 * case(name)[3] + 32 + 4 * s["max_ublocks"]) * 8
        assert s["scaled"] == 1 and s["park"] == int(lds <= 65536)
    assert built("ragged")["park"] == 1 and built("big")["park"] == 0
    assert built("ragged")["order"].size > 0 and len(set(np.diff(case("ragged")[2]).tolist())) > 1
    assert built("ragged")["n_int"] > 0 and built("ragged")["n_bnd"] > 0           # (under the box-face rule)
    assert built("wave")["n_int"] == 1 and built("wave")["max_rows"] <= 64
    assert built("minc_split")["split"].size > 0 and (built("minc_split")["split"] >> 16).max() < 15
    assert built("minc_nlu4")["max_nlu"] == 4 and built("rows")["max_nlu"] <= 3
    assert built("big")["max_rows"] == 1280 and built("big")["ord_f"].size == 2560
    assert built("two_ranks")["sub_int"].size > 0 and case("two_ranks")[1].max() >= len(case("two_ranks")[0]) - 1
    assert twin("triangle").elimination_updates_an_offdiagonal_block() and not twin("ragged").elimination_updates_an_offdiagonal_block()
    # equal bricks: no launch order, on a schedule that could have one
    assert (twin("rows").cost() == twin("rows").cost()[0]).all() and not built("rows")["big"] and built("rows")["order"].size == 0
    assert np.diff(case("wide")[0]).max() > 8 and built("wide")["infow"].size > 0 and built("wide")["ord_f"].size > 0
    assert ((built("asymmetric")["tslot"] & 15) == 15).any()


def test_build_switches_select_as_the_fallback_build_does(program, tmp_path):
    """ilu_general: the stored factor everywhere, so neither the parked nor the rows / wave kernels; pc_rows 0 / 1 forces
    the rows kernel off / on (2 x 2 blocks too); pc_wave 0 builds without the wave kernel"""
    rp, ci, sub, np_, opts = case("wave")
    s = schedule(program, tmp_path, rp, ci, sub, np_, **dict(opts, ilu_general=1, pc_rows=0, pc_wave=0))
    assert (s["diag_only"], s["rows_kernel"], s["wave_kernel"], s["park_serves"]) == (0, 0, 0, 0)
    s = schedule(program, tmp_path, rp, ci, sub, np_, **dict(opts, pc_wave=0))
    assert (s["diag_only"], s["rows_kernel"], s["wave_kernel"]) == (1, 1, 0)
    s = schedule(program, tmp_path, rp, ci, sub, np_, **dict(opts, pc_rows=0))
    assert (s["diag_only"], s["rows_kernel"], s["wave_kernel"]) == (1, 0, 0)
    rp, ci, sub, np_, opts = case("ragged")
    s = schedule(program, tmp_path, rp, ci, sub, np_, **dict(opts, pc_rows=1))
    assert (s["rows_kernel"], s["wave_kernel"], s["park_serves"]) == (1, 0, 1) and s["c16"].size > 0
    s = schedule(program, tmp_path, rp, ci, sub, np_, **dict(opts, ilu_general=1))
    assert (s["diag_only"], s["park_serves"]) == (0, 0) and s["c16"].size == 0 and s["n_templates"] == 0


def chain(n):
    rows = [[j for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)]
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.concatenate(rows)


def test_schedule_refusals_and_their_texts(program, tmp_path):
    rp, ci = chain(8)
    assert schedule(program, tmp_path, rp, ci, [0, 4, 7], 2) == {"error": "sub_ptr must cover [0, n_owned]"}
    assert schedule(program, tmp_path, rp, ci, [1, 4, 8], 2) == {"error": "sub_ptr must cover [0, n_owned]"}
    assert schedule(program, tmp_path, rp, ci, [0, 5, 3, 8], 2) == {"error": "sub_ptr not monotone"}
    rp, ci = chain(1024)
    assert schedule(program, tmp_path, rp, ci, [0, 1024], 2) == {"error": "more than 1023 dependency levels in a subdomain"}
    rp, ci = chain(1023)
    s = schedule(program, tmp_path, rp, ci, [0, 1023], 2)
    assert s["max_lev"] == 1023 and not s["big"] and ((s["info"] & 0xffffffff) >> 22).max() == 1022


# ---- the extended pattern -----------------------------------------------------------------------------------------------
def extended(program, tmp_path, rp, ci, sub, overlap, levels, sublu=0, n=None, **more):
    n = len(rp) - 1 if n is None else n
    return run(program, tmp_path, "asm", rowptr=rp, colidx=ci, sub=sub, N=n, overlap=overlap, levels=levels, sublu=sublu, **more)


def check_extended(p, rp, ci, sub, ref):
    """the program's arrays against an asm_reference.AsmPattern (entries of (rp, ci) named by plane position slot * n + row)"""
    n = len(rp) - 1
    np.testing.assert_array_equal(p["ext_ptr"], ref.ext_ptr)
    np.testing.assert_array_equal(p["ext_rows"], ref.ext_row)
    np.testing.assert_array_equal(p["ext_row"] & 0x7fffffff, ref.ext_row)
    np.testing.assert_array_equal((p["ext_row"] & 0xffffffff) >> 31, ref.owned)       # the ownership bit
    np.testing.assert_array_equal(p["erp"], ref.erp)
    np.testing.assert_array_equal(p["ecol"], ref.eci)
    row_of = np.repeat(np.arange(n), np.diff(rp))
    plane = (np.arange(rp[-1]) - rp[row_of]) * n + row_of
    want_src = np.where(ref.esrc >= 0, plane[np.maximum(ref.esrc, 0)], -1)
    np.testing.assert_array_equal(p["esrc"], want_src)
    n_ext, W = len(ref.ext_row), p["W"]
    assert W == ref.width == np.diff(ref.erp).max()
    ell, gmap = p["ell_col"].reshape(W, n_ext), p["gmap"].reshape(W, n_ext)
    want_col, want_map = np.tile(np.arange(n_ext), (W, 1)), np.full((W, n_ext), -1)    # padding: the row itself, no source
    q = np.repeat(np.arange(n_ext), np.diff(ref.erp))
    t = np.arange(ref.erp[-1]) - ref.erp[q]
    want_col[t, q], want_map[t, q] = ref.eci, want_src
    np.testing.assert_array_equal(ell, want_col)
    np.testing.assert_array_equal(gmap, want_map)


def asm_case(cid):
    eos, dims, brick, overlap, levels = ar.TOO_BIG if cid == "too_big" else ar.CASES[cid]
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos)
    return pattern(lm) + (np.asarray(lm.sub_ptr, dtype=np.int64), overlap, levels)


@pytest.mark.parametrize("cid", sorted(ar.CASES) + ["too_big"])
def test_extended_pattern_matches_the_reference_twins(program, tmp_path, cid):
    rp, ci, sub, overlap, levels = asm_case(cid)
    p = extended(program, tmp_path, rp, ci, sub, overlap, levels)
    ref = ar.AsmPattern(rp, ci, sub, overlap, levels)
    check_extended(p, rp, ci, sub, ref)
    # E's schedule as build_asm asks for it when the launch is to be fused: wide where every block fits a workgroup
    bs = {"w": 1, "we": 2, "wce": 3, "wsce": 4}[(ar.TOO_BIG if cid == "too_big" else ar.CASES[cid])[0]]
    s = schedule(program, tmp_path, p["erp"], p["ecol"], p["ext_ptr"], bs, ghosts=0, fill=1, mesh_W=int(np.diff(rp).max()))
    assert s["max_rows"] == ref.max_rows
    if cid == "too_big":
        assert ref.max_rows == ar.interior_rows(16, 16, 2) == 1152 and (s["wide"], s["big"]) == (0, 1)
    else:
        assert (s["wide"], s["big"]) == (1, 0) and s["infow"].size == len(ref.ext_row)


@pytest.mark.parametrize("overlap", [0, 1])
def test_sub_lu_complete_fill(program, tmp_path, overlap):
    """sub-preconditioner lu: every level of fill kept -- iluk_pattern with a huge level on the same blocks"""
    rp, ci, sub, np_, opts = case("rows")
    p = extended(program, tmp_path, rp, ci, sub, overlap, 0, sublu=1)
    ref = ar.AsmPattern(rp, ci, sub, overlap)
    rpf, cif, src, width = iluk_pattern(ref.erp, ref.eci, ref.ext_ptr, 1 << 20)
    ref.esrc = np.where(src >= 0, ref.esrc[np.maximum(src, 0)], -1)
    ref.erp, ref.eci, ref.width = rpf, cif, int(width)
    assert width > np.diff(rp).max()
    check_extended(p, rp, ci, sub, ref)


def test_ghost_rows_enter_the_overlap(program, tmp_path):
    """two ranks: the overlapped sets take in partition-ghost cells, whose rows come as a CSR of their own with the sender's
    slot of every entry; their blocks are named -(2 + slot * H + ghost)"""
    g, lm, prim, region = make_case(dims=(8, 8, 4), brick=(4, 4, 2), eos="we", part=(2, 1, 1))
    rp, ci = pattern(lm)
    n, H = lm.n_owned, lm.n_halo
    assert H > 0
    # a ghost cell's row: itself and the owned cells it touches, ascending; sender's slots: any distinct numbers
    grows = [sorted({n + h} | {int(i) for i in range(n) if n + h in ci[rp[i]:rp[i + 1]]}) for h in range(H)]
    grp = np.concatenate([[0], np.cumsum([len(r) for r in grows])])
    gci = np.concatenate(grows)
    gslot = np.concatenate([np.arange(len(r))[::-1] for r in grows])
    sub = np.asarray(lm.sub_ptr, dtype=np.int64)
    p = extended(program, tmp_path, rp, ci, sub, 1, 0, n=n, grp=grp, gci=gci, gslot=gslot)
    full_rp, full_ci = np.concatenate([rp, rp[-1] + grp[1:]]), np.concatenate([ci, gci])      # the local matrix, ghost rows below
    ref = ar.AsmPattern.__new__(ar.AsmPattern)
    ref.ext_ptr, ref.ext_row, ref.owned = ar.extended_sets(full_rp, full_ci, sub, 1)
    erp, eci, esrc = ar.extended_pattern(full_rp, full_ci, ref.ext_ptr, ref.ext_row)
    assert (ref.ext_row >= n).any()
    np.testing.assert_array_equal(p["ext_rows"], ref.ext_row)
    np.testing.assert_array_equal((p["ext_row"] & 0xffffffff) >> 31, ref.owned)
    np.testing.assert_array_equal(p["erp"], erp)
    np.testing.assert_array_equal(p["ecol"], eci)
    row_of = np.repeat(np.arange(n + H), np.diff(full_rp))[esrc]
    owned_src = (esrc - full_rp[row_of]) * n + row_of
    ghost_src = -(2 + gslot[np.maximum(esrc - rp[-1], 0)] * H + (row_of - n))
    np.testing.assert_array_equal(p["esrc"], np.where(row_of < n, owned_src, ghost_src))


def test_network_pairs(program, tmp_path):
    """the network's cells that share a row set are coupled pairwise: entries without a source where the cells are no
    neighbours, and net_pos / net_pair name where every pair's block lands"""
    rp, ci, sub, np_, opts = case("rows")
    brick0 = set(range(int(sub[1])))
    nbr = min(set(ci[rp[0]:rp[1]].tolist()) & brick0 - {0})
    far = max(brick0 - set(ci[rp[0]:rp[1]].tolist()))
    cells = sorted([0, nbr, far]) + [int(sub[1]) + 3]          # three in brick 0 (0 and nbr are neighbours, 0 and far not), one alone in brick 1
    a, b, c = cells.index(0), cells.index(nbr), cells.index(far)
    p = extended(program, tmp_path, rp, ci, sub, 0, 0, net_cells=cells)
    n = len(rp) - 1
    W = p["W"]
    ell = p["ell_col"].reshape(W, n)
    pairs = {}
    for pos, pair in zip(p["net_pos"].tolist(), p["net_pair"].tolist()):
        t, q = divmod(pos, n)
        assert (p["ext_rows"][q], p["ext_rows"][ell[t, q]]) == (cells[pair // 4], cells[pair % 4])
        pairs[pair] = p["gmap"].reshape(W, n)[t, q]
    assert sorted(pairs) == [4 * a + b for a in range(3) for b in range(3)] + [15]
    assert pairs[a * 4 + c] == -1 and pairs[c * 4 + a] == -1 and pairs[a * 4 + b] >= 0 and pairs[b * 4 + a] >= 0 and pairs[a * 4 + a] >= 0


def star(leaves):
    rows = [list(range(leaves + 1))] + [[0, i] for i in range(1, leaves + 1)]
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.concatenate(rows)


def test_extended_refusals_and_their_texts(program, tmp_path):
    """a hub that comes first fills every leaf's row completely: 257 blocks with 256 leaves"""
    rp, ci = star(256)
    assert extended(program, tmp_path, rp, ci, [0, 257], 0, 0, sublu=1) == {
        "error": "sub-preconditioner lu: the complete fill of a block gives a factor row of 257 blocks or more, the cap is 255 "
                 "(smaller subdomains, or sub-preconditioner ilu)"}
    assert extended(program, tmp_path, rp, ci, [0, 257], 0, 1) == {"error": "ILU(k): more than 255 blocks in a factor row"}
    rp, ci = star(254)               # 255 blocks: accepted, the last leaf's row is full
    p = extended(program, tmp_path, rp, ci, [0, 255], 0, 0, sublu=1)
    assert p["W"] == 255 and np.diff(p["erp"])[-1] == 255
