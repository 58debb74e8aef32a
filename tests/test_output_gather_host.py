"""The device-free halves of the N-rank output file (waiwera_amd/partition.py, waiwera_amd/simulation.py): which rank
contributes a face that two ranks hold, and the datasets of the file from a list of snapshots."""
import json
import os

import numpy as np
import pytest

from tests.test_input_partition import INPUTS, RecordingOde
from waiwera_amd.partition import face_owner, partition_mesh
from waiwera_amd.simulation import Simulation, output_datasets


def _whole_mesh():
    """model intercomparison problem 5a's gmsh mesh: 96 cells, Dirichlet boundary cells behind one edge"""
    inp = json.load(open(os.path.join(INPUTS, "problem5a.json")))
    lm = Simulation(inp, base_dir=INPUTS, ode_factory=RecordingOde).mesh
    assert lm.n_bc > 0 and lm.n_halo == 0
    return lm


@pytest.mark.parametrize("world,kind", [(2, "blocks"), (3, "blocks"), (2, "stripes"), (3, "stripes")])
def test_every_face_is_contributed_by_exactly_one_rank(world, kind):
    """contiguous blocks of cells, and cells dealt out in turn (nearly every face then lies between two ranks): every face
    of the whole mesh is owned once, by a rank that holds it; a face between two ranks is held by both; a boundary face
    goes with its cell; and the local faces' cells, turned where face_flip says so, are the whole mesh's"""
    lm = _whole_mesh()
    N = lm.n_owned
    owner = (np.arange(N) * world) // N if kind == "blocks" else np.arange(N) % world
    fc = np.asarray(lm.face_cells).reshape(-1, 2)
    fo = face_owner(fc, owner)
    interior = np.where(fc[:, 0] < N, fc[:, 0], fc[:, 1])
    assert np.array_equal(fo[fc[:, 1] >= N], owner[interior[fc[:, 1] >= N]])           # boundary faces: with their cell
    assert np.array_equal(fo[fc[:, 1] < N], owner[fc[fc[:, 1] < N, 0]])                # the others: cell 1's rank
    owned, held = np.zeros(lm.n_faces, dtype=int), np.zeros(lm.n_faces, dtype=int)
    for rank in range(world):
        m, gid = partition_mesh(lm, owner, rank, world=world)
        ex = m.extras
        fg, flip, mine = np.asarray(ex["face_gid"]), np.asarray(ex["face_flip"]), np.asarray(ex["face_owned"])
        assert fg.shape == flip.shape == mine.shape == (m.n_faces,) and len(set(fg.tolist())) == m.n_faces
        held[fg] += 1
        owned[fg[mine]] += 1
        assert np.array_equal(mine, fo[fg] == rank)
        # local cell -> whole-mesh cell: owned and ghost cells through gid, boundary cells through their one-rank index
        to_whole = np.concatenate([gid, N + np.asarray(ex.get("bc_global_index", np.zeros(0, dtype=np.int64)))])
        lf = to_whole[np.asarray(m.face_cells).reshape(-1, 2)]
        lf = np.where(flip[:, None], lf[:, ::-1], lf)
        assert np.array_equal(lf, fc[fg])
    assert (owned == 1).all()
    between = (fc[:, 1] < N) & (owner[np.clip(fc[:, 0], 0, N - 1)] != owner[np.clip(fc[:, 1], 0, N - 1)])
    assert between.any() and np.array_equal(held, np.where(between, 2, 1))


def test_a_boundary_face_goes_with_its_cell_on_either_side():
    owner = np.array([0, 1, 1])
    fc = np.array([[0, 1], [1, 2], [2, 3], [4, 0]])      # cells 3 and 4 are boundary cells; the last face lists its first
    assert face_owner(fc, owner).tolist() == [0, 1, 1, 0]
    with pytest.raises(ValueError, match="face 1 joins two boundary cells"):
        face_owner(np.array([[0, 1], [3, 4]]), owner)


def test_output_datasets_of_hand_made_snapshots():
    """the dictionary save_hdf5 has written from a one-rank run's snapshots, path by path: per-snapshot fields stacked,
    geometry and the faces' cells taken once, sources and network nodes under /source_fields, MINC level and parent only
    where given"""
    def snap(t):
        return {"time": t, "fluid_pressure": np.array([1.0, 2.0, 3.0]) + t, "cell_geometry_centroid": np.arange(6.0).reshape(3, 2),
                "cell_geometry_volume": np.array([5.0, 6.0, 7.0]), "tracer_a": np.array([0.1, 0.2, 0.3]) * t,
                "source_rate": np.array([-1.0, 2.0]) * t, "flux_water": np.array([0.5, -0.5]) + t,
                "face_cell_1": np.array([0, 1]), "face_cell_2": np.array([1, -1]), "face_geometry_area": np.array([10.0, 20.0]),
                "network_group_rate": np.array([-3.0]) - t}
    outs = [snap(0.0), snap(2.0)]
    want = {
        "/time": np.array([[0.0], [2.0]]),
        "/cell_index": np.array([[0], [1], [2]], dtype=np.int32),
        "/cell_fields/fluid_pressure": np.array([[1.0, 2.0, 3.0], [3.0, 4.0, 5.0]]),
        "/cell_fields/cell_geometry_centroid": np.arange(6.0).reshape(3, 2),
        "/cell_fields/cell_geometry_volume": np.array([5.0, 6.0, 7.0]),
        "/cell_fields/tracer_a": np.array([[0.0, 0.0, 0.0], [0.2, 0.4, 0.6]]),
        "/source_fields/source_rate": np.array([[-0.0, 0.0], [-2.0, 4.0]]),
        "/face_fields/flux_water": np.array([[0.5, -0.5], [2.5, 1.5]]),
        "/face_cell_1": np.array([[0], [1]], dtype=np.int32),
        "/face_cell_2": np.array([[1], [-1]], dtype=np.int32),
        "/face_fields/face_geometry_area": np.array([10.0, 20.0]),
        "/source_fields/network_group_rate": np.array([[-3.0], [-5.0]]),
    }
    got = output_datasets(outs, 3)
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    minc = output_datasets(outs, 3, np.array([0, 0, 1]), np.array([0, 1, 1]))
    assert list(minc)[:4] == ["/time", "/cell_index", "/minc/level", "/minc/parent"]
    assert minc["/minc/level"].dtype == np.int32 and minc["/minc/level"].tolist() == [[0], [0], [1]]
    assert minc["/minc/parent"].tolist() == [[0], [1], [1]]
    assert all(np.array_equal(minc[k], got[k]) for k in got)
