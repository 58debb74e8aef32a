"""Host side of meshes whose cells have more than 8 faces: MULgraph columns of any number of nodes, n-gon prisms in
unstructured.build_mesh, and the CPU oracle's time step on a mesh whose coarse columns border twelve fine ones
(tests/wide_mesh.py).  No GPU."""
import os
import sys

import numpy as np

from oracle import binding as ol
from waiwera_amd import mulgrid, unstructured
from waiwera_amd.cases import scaled

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_mesh as wm  # noqa: E402


def strip_plan(h=100.0):
    """eight unit-square columns in a row; column q has q + 1 extra nodes on its outer (y = 0) edge: 5 .. 12 nodes"""
    xy, columns, names = [], [], {}

    def node(x, y):
        if (x, y) not in names:
            names[(x, y)] = len(xy)
            xy.append((x * h, y * h))
        return names[(x, y)]

    for q in range(8):
        extra = q + 1
        ring = [node(q, 0)] + [node(q + (t + 1) / (extra + 1.0), 0) for t in range(extra)]
        ring += [node(q + 1, 0), node(q + 1, 1), node(q, 1)]
        columns.append(ring)
    return np.array(xy), columns


def test_mulgraph_polygon_columns(tmp_path):
    xy, columns = strip_plan()
    assert [len(c) for c in columns] == list(range(5, 13))
    path = os.path.join(str(tmp_path), "gpoly.dat")
    wm.write_mulgraph(path, xy, columns, [0.0, -50.0, -150.0])
    nodes, cells, dim = mulgrid.read_geometry(path)
    assert dim == 3 and len(cells) == 16
    assert [len(c) for c in cells[:8]] == [2 * k for k in range(5, 13)]
    lm = unstructured.build_mesh(nodes, cells, 3, gravity=[0.0, 0.0, -9.8])
    vol = lm.cell_geom[:16, 3]
    assert np.allclose(vol[:8], 100.0 * 100.0 * 50.0) and np.allclose(vol[8:], 100.0 * 100.0 * 100.0)
    assert np.allclose(lm.cell_geom[3, :3], [350.0, 50.0, -25.0])
    assert lm.n_faces == 2 * 7 + 8          # in-layer faces + faces between the layers


def test_ngon_prisms():
    """n-gon prisms of the refined plan: volume = plan area x thickness, each cell's outward area vectors sum to zero,
    the coarse cells have 12 lateral faces"""
    xy, columns, coarse = wm.refined_plan()
    tops = [0.0, -80.0, -200.0]
    nodes, cells = wm.layered_cells(xy, columns, tops)
    nc = len(columns)
    assert sorted({len(c) for c in columns}) == [4, 12] and all(len(columns[q]) == 12 for q in coarse)
    area = np.array([unstructured._polygon(xy[c])[0] for c in columns])
    lm = unstructured.build_mesh(nodes, cells, 3)
    vol = lm.cell_geom[: len(cells), 3]
    assert np.allclose(vol[:nc], area * 80.0, rtol=1e-12) and np.allclose(vol[nc:], area * 120.0, rtol=1e-12)
    for nd in cells:
        p = nodes[nd]
        c0 = p.mean(axis=0)
        tot = np.zeros(3)
        for f in unstructured._cell_faces(len(nd)):
            av, fc = unstructured._face3d(p[list(f)])
            tot += av if np.dot(fc - c0, av) > 0 else -av
        assert np.abs(tot).max() < 1e-9 * np.abs(p).max() ** 2
    assert len(unstructured._cell_faces(24)) == 14
    fc = lm.face_cells
    for q in coarse:
        for lay in range(2):
            c = lay * nc + q
            others = np.concatenate([fc[fc[:, 0] == c, 1], fc[fc[:, 1] == c, 0]])
            same_layer = [o for o in others if lay * nc <= o < (lay + 1) * nc]
            assert len(same_layer) == 12 and len(others) == 13
    # the existing shapes keep their tables: a hexahedron's faces are HEX_FACES
    assert unstructured._cell_faces(8) is unstructured.HEX_FACES and unstructured._cell_faces(6) is unstructured.PRISM_FACES


def test_oracle_time_step_on_wide_mesh_keeps_balance(oracle):
    """a closed box with sources: the mass the step adds up equals what the sources put in"""
    eos, dt = "we", 2.0e4
    lm, prim, region, coarse = wm.wide_case(eos, top_bc=False)
    n = lm.n_owned
    fc = lm.face_cells
    deg = np.bincount(fc.ravel(), minlength=n)[:n]
    assert deg.max() == 14
    osim = ol.OracleSim(oracle, lm, 1)
    osim.set_regions(region)
    yo = osim.yvec(scaled(prim, region, eos).ravel().copy())
    assert osim.pre_eval(yo) == 0
    L0 = osim.lhs()[: 2 * n].reshape(n, 2).copy()
    o = osim.opts()
    o.ksp_rtol, o.ftol_rel = 1e-12, 1e-11
    r, nits = osim.timestep(yo, dt, o)
    assert r > 0 and nits >= 1
    assert osim.pre_eval(yo) == 0
    L1 = osim.lhs()[: 2 * n].reshape(n, 2)
    V = lm.cell_geom[:n, 3]
    dm = ((L1[:, 0] - L0[:, 0]) * V).sum()
    src = lm.src_rate.sum() * dt
    assert abs(dm - src) < 1e-6 * np.abs(lm.src_rate).sum() * dt, (dm, src)
    osim.close()
