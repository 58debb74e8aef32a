"""What the compact-cell-order tests share: layered hex grids as centroids and faces, the ordering written in numpy from
its definition (include/waiwera_hip.h, wai_cell_order), cut shares and in-subdomain coupling counts of a numbering, and
the same grids as gmsh 2.2 ASCII files."""
import numpy as np


def hex_grid(nx, ny, nz, spacing=(100.0, 100.0, 20.0), jitter=0.0, seed=0):
    """centroids (n, 3) numbered x fastest / z slowest and the interior faces (m, 2): x faces, then y, then z.  jitter:
    the horizontal coordinates moved by a seeded +- that share of the spacing"""
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cen = np.stack([(i.ravel() + 0.5) * spacing[0], (j.ravel() + 0.5) * spacing[1], (k.ravel() + 0.5) * spacing[2]], axis=1)
    if jitter:
        rng = np.random.default_rng(seed)
        cen[:, :2] += rng.uniform(-jitter, jitter, size=(len(cen), 2)) * np.asarray(spacing[:2])
    idx = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    faces = np.concatenate([np.stack([idx[:, :, :-1].ravel(), idx[:, :, 1:].ravel()], axis=1),
                            np.stack([idx[:, :-1, :].ravel(), idx[:, 1:, :].ravel()], axis=1),
                            np.stack([idx[:-1, :, :].ravel(), idx[1:, :, :].ravel()], axis=1)])
    return cen, faces.astype(np.int64)


def scramble(cen, faces, seed):
    """the same mesh as another file would number it: cell k of the result is cell p[k] of the given one; the faces in
    another order too, some of them turned round.  Returns (cen, faces, p)"""
    rng = np.random.default_rng(seed)
    p = rng.permutation(len(cen))
    inv = np.empty_like(p)
    inv[p] = np.arange(len(p))
    f = inv[faces][rng.permutation(len(faces))]
    turn = rng.random(len(f)) < 0.5
    f[turn] = f[turn][:, ::-1]
    return cen[p].copy(), f, p


def spacings(cen, faces):
    """(h, has_faces) per axis: the mean centroid distance over the faces of that axis, summed in face order"""
    h, has = np.ones(3), [False] * 3
    if len(faces):
        d = np.abs(cen[faces[:, 0]] - cen[faces[:, 1]])
        ax = np.argmax(d, axis=1)              # the first maximum: ties go to the lowest axis
        for a in range(3):
            sel = d[ax == a, a]
            has[a] = len(sel) > 0
            h[a] = np.cumsum(sel)[-1] / len(sel) if len(sel) else 1.0     # cumsum: a sequential sum
    return h, has


def _sorted(cells, cen, a):
    """cells by c[.][a], then the remaining axes in the order z, y, x, then the index"""
    rest = [b for b in (2, 1, 0) if b != a]
    keys = [cells] + [cen[cells, b] for b in reversed(rest)] + [cen[cells, a]]
    return cells[np.lexsort(keys)]


def compact_order(cen, faces, S):
    """(perm with perm[new] = old, sub_ptr) from the definition"""
    h, has = spacings(cen, faces)
    leaves = []

    def bisect(cells):
        k = len(cells)
        L = -(-k // S)
        if L <= 1:
            leaves.append(_sorted(cells, cen, 2))
            return
        best, ebest = 0, None
        for a in range(3):
            e = np.float64(0.0)
            if not len(faces) or has[a]:
                with np.errstate(all="ignore"):
                    e = (cen[cells, a].max() - cen[cells, a].min()) / np.float64(h[a])
            if a == 0 or e > ebest:
                best, ebest = a, e
        cells = _sorted(cells, cen, best)
        left = k * (L // 2) // L
        bisect(cells[:left])
        bisect(cells[left:])
    if len(cen):
        bisect(np.arange(len(cen)))
    perm = np.concatenate(leaves) if leaves else np.zeros(0, dtype=np.int64)
    return perm, np.concatenate([[0], np.cumsum([len(x) for x in leaves])]).astype(np.int64)


def renumbered(cen, faces, perm):
    """the mesh numbered by perm[new] = old; the faces keep their order"""
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    return cen[perm].copy(), inv[faces]


def cut_share(faces, sub_ptr):
    """share of the faces whose two cells lie in different subdomains of the numbering the faces are given in"""
    owner = np.repeat(np.arange(len(sub_ptr) - 1), np.diff(sub_ptr))
    return float(np.mean(owner[faces[:, 0]] != owner[faces[:, 1]]))


def coupling_counts(faces, sub_ptr):
    """(most lower, most upper) in-subdomain couplings of any row"""
    n = int(sub_ptr[-1])
    owner = np.repeat(np.arange(len(sub_ptr) - 1), np.diff(sub_ptr))
    f = faces[owner[faces[:, 0]] == owner[faces[:, 1]]]
    lo, hi = f.min(axis=1), f.max(axis=1)
    return int(np.bincount(hi, minlength=n).max()), int(np.bincount(lo, minlength=n).max())


def chunks(n, S):
    return np.append(np.arange(0, n, S), n)


def write_msh(path, nx, ny, nz, spacing=(100.0, 100.0, 20.0), order=None):
    """the hex grid as a gmsh 2.2 ASCII file; order: element k of the file is cell order[k] of the x-fastest numbering"""
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    xyz = np.stack([i.ravel() * spacing[0], j.ravel() * spacing[1], k.ravel() * spacing[2]], axis=1)
    node = np.arange((nx + 1) * (ny + 1) * (nz + 1)).reshape(nz + 1, ny + 1, nx + 1) + 1
    elems = []
    for c in (range(nx * ny * nz) if order is None else order):
        i0, j0, k0 = int(c) % nx, (int(c) // nx) % ny, int(c) // (nx * ny)
        elems.append([node[k0, j0, i0], node[k0, j0, i0 + 1], node[k0, j0 + 1, i0 + 1], node[k0, j0 + 1, i0],
                      node[k0 + 1, j0, i0], node[k0 + 1, j0, i0 + 1], node[k0 + 1, j0 + 1, i0 + 1], node[k0 + 1, j0 + 1, i0]])
    with open(path, "w") as f:
        f.write("$MeshFormat\n2.2 0 8\n$EndMeshFormat\n$Nodes\n%d\n" % len(xyz))
        for q, p in enumerate(xyz):
            f.write("%d %.17g %.17g %.17g\n" % (q + 1, p[0], p[1], p[2]))
        f.write("$EndNodes\n$Elements\n%d\n" % len(elems))
        for q, e in enumerate(elems):
            f.write("%d 5 2 1 1 %s\n" % (q + 1, " ".join(str(int(v)) for v in e)))
        f.write("$EndElements\n")
    return str(path)


def layered_input(nx, ny, nz, filename, number=None, eos="we", step=2.0e5):
    """an input on the nx x ny x nz hex grid with everything that carries a cell number: boundaries at the top layer, two
    sources, a rock type given by cells and one by a zone given as a cell list, per-cell initial conditions (hydrostatic,
    warming with depth).  number[c]: the file's number of the x-fastest cell c (None: the x-fastest numbering itself);
    per-cell arrays are listed in the file's numbering"""
    n = nx * ny * nz
    number = np.arange(n) if number is None else np.asarray(number)
    where = np.empty(n, dtype=np.int64)      # where[file number] = x-fastest cell
    where[number] = np.arange(n)
    k = np.arange(n) // (nx * ny)
    depth = (nz - 0.5 - k) * 20.0
    primary = np.stack([1.0e5 + 9.0e3 * depth, 20.0 + 0.25 * depth] + ([np.full(n, 1.0e3)] if eos == "wce" else []), axis=1)
    top = np.arange(n - nx * ny, n)
    low = np.arange(0, nx * ny * 2)                       # the two lowest layers: tighter rock, by cells
    lens = np.nonzero((k >= 3) & (k <= 5) & (np.arange(n) % nx < nx // 2))[0]      # a lens, by a zone given as a cell list
    cell = lambda cells: [int(number[c]) for c in np.atleast_1d(cells)]      # noqa: E731
    return {
        "mesh": {"filename": filename, "zones": {"lens": {"cells": cell(lens)}}},
        "eos": {"name": eos}, "gravity": 9.8,
        "rock": {"types": [{"name": "base", "permeability": [1.0e-13, 1.0e-13, 2.0e-14], "porosity": 0.1, "zones": "all"},
                           {"name": "tight", "permeability": [2.0e-14, 2.0e-14, 5.0e-15], "porosity": 0.08, "cells": cell(low)},
                           {"name": "lens", "permeability": [5.0e-13, 5.0e-13, 1.0e-13], "porosity": 0.2, "zones": ["lens"]}]},
        "initial": {"primary": primary[where].tolist(), "region": [1] * n},
        "boundaries": [{"primary": [1.0e5, 20.0] + ([1.0e3] if eos == "wce" else []), "region": 1,
                        "faces": {"cells": cell(top), "normal": [0, 0, 1]}}],
        "source": [{"cell": cell(nx // 3 + nx * (ny // 2) + nx * ny * 1)[0], "rate": 2.0, "enthalpy": 4.0e5},
                   {"cell": cell(n - 1 - nx * ny * 2 - nx)[0], "rate": -1.0}],
        "time": {"start": 0.0, "stop": step, "step": {"size": step, "maximum": {"number": 1},
                                                      "solver": {"nonlinear": {"maximum": {"iterations": 12}}}}},
        "output": False,
    }
