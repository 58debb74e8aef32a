"""The library's own pattern is the one tests/test_mesh_pattern_host.py checks on the host: a context created on the
3 x 2 x 1 box with boundary cells returns exactly the rowptr and colidx of that test's numpy construction."""
import ctypes as C

import numpy as np
import pytest

from tests.test_mesh_pattern_host import box_3x2, twin
from waiwera_amd import lib as wl

pytestmark = pytest.mark.gpu


def test_context_pattern_is_the_host_builders():
    n_owned, n_halo, n_bc, faces = box_3x2()
    want = twin(n_owned, n_halo, n_bc, faces)
    n_local, n_faces = n_owned + n_halo + n_bc, len(faces)
    face_geom = np.zeros((n_faces, 12))
    face_geom[:, 0], face_geom[:, 1:3], face_geom[:, 3] = 100.0, 5.0, 10.0     # area, the two distances, their sum
    face_geom[:, 11] = [1, 1, 1, 1, 2, 2, 2, 1, 1]                               # permeability direction
    cell_geom = np.tile([0.0, 0.0, 0.0, 1000.0], (n_local, 1))                  # (centroid, volume)
    rock = np.tile([1.e-13, 1.e-13, 1.e-13, 2.5, 2.5, 0.1, 2600.0, 900.0], (n_local, 1))
    keep = (wl._i32(np.ravel(faces)), wl._f64(face_geom), wl._f64(cell_geom), wl._f64(rock))
    md = wl.MeshDesc()
    md.n_owned, md.n_halo, md.n_bc, md.n_faces = n_owned, n_halo, n_bc, n_faces
    md.face_cells, md.face_geom = keep[0].ctypes.data_as(wl.pi), keep[1].ctypes.data_as(wl.pd)
    md.cell_geom, md.rock = keep[2].ctypes.data_as(wl.pd), keep[3].ctypes.data_as(wl.pd)
    eos, opts, h = wl.eos_desc("we"), wl.default_opts(), C.c_void_p()
    rc = wl.LIB.wai_ctx_create(C.byref(md), C.byref(eos), C.byref(opts), 0, C.byref(h))
    try:
        assert rc == 0, wl.LIB.wai_last_error(h).decode()
        assert wl.LIB.wai_jacobian_nnzb(h) == want["nnzb"]
        rowptr, colidx = np.full(n_owned + 1, -1, dtype=np.int32), np.full(want["nnzb"], -1, dtype=np.int32)
        assert wl.LIB.wai_jacobian_pattern(h, rowptr.ctypes.data_as(wl.pi), colidx.ctypes.data_as(wl.pi)) == 0
        np.testing.assert_array_equal(rowptr, want["rowptr"])
        np.testing.assert_array_equal(colidx, want["colidx"])
    finally:
        assert wl.LIB.wai_ctx_destroy(h) == 0
