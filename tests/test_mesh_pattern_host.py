"""The mesh -> pattern construction of wai_ctx_create (csrc/mesh_pattern.hpp) without a GPU: a stand-alone program
(tests/mesh_pattern_host/main.cpp) built with the address and undefined-behaviour sanitizers calls build_mesh_pattern on
small meshes; every array it prints is compared with an independent construction in numpy (`twin`: sorted sets of
neighbours per cell), and its refusals with their texts."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("adj_face", "adj_other", "adj_blk", "adj_tblk", "diag", "rowptr", "colidx", "ell_col")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mesh_pattern_host") / "mesh_pattern_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "waiwera_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mesh_pattern_host", "main.cpp"), "-o", str(exe)])
    return str(exe)


def run(program, tmp_path, n_owned, n_halo, n_bc, faces):
    """what the program prints for a mesh: {"error": text} or {name: value(s)}; it exits 0 either way"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 2)
    mesh = tmp_path / "mesh.txt"
    mesh.write_text("%d %d %d %d\n" % (n_owned, n_halo, n_bc, len(faces)) + "".join("%d %d\n" % tuple(f) for f in faces))
    p = subprocess.run([program, str(mesh)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = {}
    for line in p.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "error":
            code, _, text = rest.partition(" ")
            assert int(code) == -2
            return {"error": text}
        vals = np.array(rest.split(), dtype=np.int64)
        out[name] = vals if name in ARRAYS else int(vals[0])
    return out


def twin(n_owned, n_halo, n_bc, faces):
    """the same arrays from the definitions: a row's columns are the sorted set of the cell and its neighbours that have a
    column (owned and ghost cells); a slot is a position in that sorted set"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 2)
    n_prim = n_owned + n_halo
    # (face * 2 + side, cell across) of every face of an owned cell, ascending: slots are filled in that order
    sides = [sorted((2 * f + s, int(faces[f, 1 - s])) for f in range(len(faces)) for s in (0, 1) if faces[f, s] == i)
             for i in range(n_owned)]
    cols = [sorted({i} | {o for _, o in sides[i] if o < n_prim}) for i in range(n_owned)]
    max_deg, W = max(len(s) for s in sides), max(len(c) for c in cols)
    adj_face, adj_other = np.full((max_deg, n_owned), -1), np.zeros((max_deg, n_owned), dtype=np.int64)
    adj_blk, adj_tblk = np.full((max_deg, n_owned), -1), np.full((max_deg, n_owned), -1)
    ell_col = np.tile(np.arange(n_owned), (W, 1))          # padding: the row's own index
    for i in range(n_owned):
        for s, (fs, o) in enumerate(sides[i]):
            adj_face[s, i], adj_other[s, i] = fs, o
            if o < n_prim:
                adj_blk[s, i] = cols[i].index(o)
            if o < n_owned:
                adj_tblk[s, i] = cols[o].index(i)
        ell_col[:len(cols[i]), i] = cols[i]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    return dict(max_deg=max_deg, W=W, nnzb=int(rowptr[-1]), adj_face=adj_face.ravel(), adj_other=adj_other.ravel(),
                adj_blk=adj_blk.ravel(), adj_tblk=adj_tblk.ravel(), diag=np.array([c.index(i) for i, c in enumerate(cols)]),
                rowptr=rowptr, colidx=np.concatenate(cols), ell_col=ell_col.ravel())


def box_3x2(owned_columns=3):
    """the 3 x 2 x 1 box, cell (i, j).  All of it owned (cells i + 3 j) with two boundary cells beyond its i = 2 end; or
    cut after `owned_columns` = 2 columns: four owned cells, the i = 2 column as ghosts, no boundary cells.
    Returns n_owned, n_halo, n_bc, faces"""
    if owned_columns == 3:
        cell = {(i, j): i + 3 * j for j in range(2) for i in range(3)}
        extra, sizes = [(cell[2, 0], 6), (7, cell[2, 1])], (6, 0, 2)    # (the second boundary face with its cell on side 1)
    else:
        cell = {(i, j): i + 2 * j for j in range(2) for i in range(2)}
        cell.update({(2, 0): 4, (2, 1): 5})
        extra, sizes = [], (4, 2, 0)
    faces = [(cell[i, j], cell[i + 1, j]) for j in range(2) for i in range(2)] + [(cell[i, 0], cell[i, 1]) for i in range(3)]
    return sizes + (faces + extra,)


def star(n_owned_nbrs, n_bc_faces):
    """cell 0 with n_owned_nbrs owned neighbours (every other face with cell 0 on side 1) and n_bc_faces boundary faces"""
    faces = [(0, k) if k % 2 else (k, 0) for k in range(1, n_owned_nbrs + 1)]
    faces += [(0, n_owned_nbrs + 1 + b) for b in range(n_bc_faces)]
    return 1 + n_owned_nbrs, 0, n_bc_faces, faces


ACCEPTED = {
    "box with boundary cells": box_3x2(),
    "box cut, ghost columns": box_3x2(owned_columns=2),
    "one cell, no faces": (1, 0, 0, []),
    "star at the limit": star(15, 1),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_arrays_match_the_numpy_construction(program, tmp_path, case):
    mesh = ACCEPTED[case]
    got, want = run(program, tmp_path, *mesh), twin(*mesh)
    assert sorted(got) == sorted(want)
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def test_the_cases_reach_the_branches_they_are_for(program, tmp_path):
    """(of the twin's arrays, which the test above holds equal to the program's)"""
    box, cut, one, lim = (twin(*ACCEPTED[k]) for k in ("box with boundary cells", "box cut, ghost columns",
                                                       "one cell, no faces", "star at the limit"))
    # boundary faces have no block; cell 0's row (3 blocks) is narrower than W = 4 and padded with its own index
    assert box["W"] == 4 and (box["adj_blk"].reshape(-1, 6)[:, [2, 5]] == -1).sum() == 2
    assert box["rowptr"][1] == 3 and box["ell_col"].reshape(4, 6)[3, 0] == 0
    # ghost columns in the rows, no transposed slot towards a ghost
    assert cut["colidx"].max() == 5 and ((cut["adj_other"] >= 4) & (cut["adj_face"] >= 0) & (cut["adj_tblk"] == -1)).sum() == 2
    assert (one["W"], one["nnzb"], one["max_deg"]) == (1, 1, 0)
    assert (lim["W"], lim["max_deg"]) == (16, 16)


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_transposed_slots_point_back(program, tmp_path, case):
    """what the column-wise Jacobian sweep rests on: for an owned cell i and its owned neighbour o in slot s, slot
    adj_tblk[s, i] of row o is column i, and slot adj_blk[s, i] of row i is column o"""
    n_owned = ACCEPTED[case][0]
    p = run(program, tmp_path, *ACCEPTED[case])
    shape = (p["max_deg"], n_owned)
    face, other, blk, tblk = (p[k].reshape(shape) for k in ("adj_face", "adj_other", "adj_blk", "adj_tblk"))
    pairs = 0
    for s, i in zip(*np.nonzero((face >= 0) & (other < n_owned))):
        o = other[s, i]
        assert p["colidx"][p["rowptr"][o] + tblk[s, i]] == i
        assert p["colidx"][p["rowptr"][i] + blk[s, i]] == o
        pairs += 1
    assert pairs == sum(1 for a, b in np.reshape(ACCEPTED[case][3], (-1, 2)) if a < n_owned and b < n_owned) * 2


REFUSED = {
    "17 faces on one cell": (star(15, 2), "cell 0 has 17 faces: at most 16 supported"),
    "16 faces, all to owned cells": (star(16, 0), "cell 0 has 16 neighbouring cells (a matrix row of 17 blocks): at most 15 supported"),
    "two faces between one pair": ((2, 0, 0, [(0, 1), (1, 0)]), "duplicate connection between two cells"),
    "face cell index n_local": ((2, 0, 1, [(0, 1), (1, 3)]), "face cell index out of range"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_and_their_texts(program, tmp_path, case):
    mesh, text = REFUSED[case]
    assert run(program, tmp_path, *mesh) == {"error": text}
