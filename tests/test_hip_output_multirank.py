"""The input's HDF5 output file from a run on two ranks (waiwera_amd/simulation.py: every snapshot a collective gather to
rank 0 through wai_gather_fluid / wai_gather_rows, rank 0 writes) against the one-rank run of the same input.

Like every multi-rank test here the ranks share ONE GPU over the loop-back transport of tests/loopback_rccl: what is checked
is the front end's wiring -- every place filled once, faces sent by one rank, nothing left under a condition that differs
between ranks (that would end a case at its queue timeout) -- not RCCL between real devices.

Inputs are the reference's own (tests/golden/inputs) cut to five steps: the tracer doublet, the MINC column, and the
reinjection column asked for every flux, the sources' separated flows and the network's fields, with an initial snapshot,
one every second step and the final one.  The dictionaries of datasets (simulation.output_datasets) are compared path by
path: /time, /cell_index, /minc/*, the faces' cells and all geometry exactly -- they are copied or come from the whole mesh
-- and state, flux, source and network datasets within 1e-4 of the dataset's largest magnitude, the two-ranks-against-one
bound of tests/test_hip_input_multirank_features.py for the reason given there (both runs stop Newton at 1e-5, with
different preconditioner subdomains).  The two ranks are started once and run the three inputs one after the other, then
the doublet again with a writer that raises on rank 0.

Before the gather, a run on N ranks collected no dictionary and wrote no file: every test here fails there."""
import copy
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_hip_input_multirank_features import INPUTS, TOL, _doublet
from tests.test_hip_multirank import LOOPBACK, ROOT, _default_overlap, _free_port, _own_cus

pytestmark = pytest.mark.gpu
STEPS = 5
EXACT = ("/time", "/cell_index", "/minc/", "/face_cell_", "/cell_fields/cell_geometry", "/face_fields/face_geometry")


def _inputs():
    """{case: (input, Simulation keywords)}"""
    def cut(inp, **out):
        inp = copy.deepcopy(inp)
        inp["time"]["step"].setdefault("maximum", {})["number"] = STEPS
        inp["output"] = dict(inp.get("output") or {}, **out)
        return inp
    rj = json.load(open(os.path.join(INPUTS, "reinjection.json")))
    rj = cut(rj, filename="reinjection.h5", initial=True, frequency=2, final=True,
             fields=dict(flux=["all"], source=["rate", "enthalpy", "water_rate", "water_enthalpy", "steam_rate", "steam_enthalpy"],
                         network_group=["rate", "enthalpy", "steam_rate"],
                         network_reinject=["output_water_rate", "output_steam_rate", "overflow_water_rate"]))
    return {
        "doublet": (cut(_doublet(1), filename="doublet.h5"), {}),
        "minc": (cut(json.load(open(os.path.join(INPUTS, "minc_column_minc.json"))), filename="minc.h5"),
                 dict(mesh_file=os.path.join(INPUTS, "gminc_column.dat"))),
        "reinjection": (rj, dict(mesh_file=os.path.join(INPUTS, "greinjection.dat"))),
        "no_writer": (cut(_doublet(1), filename="doublet.h5"), {}),      # two ranks only: rank 0's writer raises (_worker)
    }


def _hdf5():
    from waiwera_amd import hdf5io
    try:
        hdf5io._lib()
        return True
    except hdf5io.Hdf5Unavailable:
        return False


def _read_back(path, data):
    from waiwera_amd import hdf5io
    return {k: hdf5io.read_dataset(path, k) for k in data}


def _worker(rank, world, uid_q, q, tmp):
    os.environ["WAI_RCCL_LIB"] = LOOPBACK
    _own_cus(rank, world)
    _default_overlap()
    from waiwera_amd import lib as wl
    from waiwera_amd.simulation import Simulation
    res = {}
    for case, (inp, kw) in _inputs().items():
        if rank == 0:
            uid = wl.comm_unique_id()
            for _ in range(world - 1):
                uid_q.put(uid)
        else:
            uid = uid_q.get(timeout=120)
        if case == "no_writer" and rank == 0:
            from waiwera_amd import hdf5io

            def refuse(path, data):
                raise hdf5io.Hdf5Unavailable("no HDF5 library")
            hdf5io.write_file = refuse                           # (the last case: nothing after it writes)
        out_dir = os.path.join(tmp, case, "rank%d" % rank)      # a directory per rank: who wrote what
        os.makedirs(out_dir)
        sim = Simulation(inp, base_dir=INPUTS, rank=rank, world=world, comm_id=uid, output_dir=out_dir, **kw)
        own = sim.run()
        data = sim.datasets()
        path = os.path.join(out_dir, inp["output"]["filename"])
        res[case] = dict(data=data, taken=sim.ts.taken, error=None if sim.output_error is None else repr(sim.output_error),
                         files=sorted(os.listdir(out_dir)), own_cells=own["fluid_pressure"].size, n_owned=sim.mesh.n_owned,
                         back=_read_back(path, data) if data is not None and os.path.exists(path) else None)
        sim.ode.destroy()
    q.put((rank, res))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """-> {case: (the one-rank run's datasets, [what each of the two ranks sent back])}"""
    from waiwera_amd.simulation import Simulation
    assert os.path.exists(LOOPBACK), "build first: python __graft_entry__.py"
    tmp = str(tmp_path_factory.mktemp("gathered_output"))
    one = {}
    for case, (inp, kw) in _inputs().items():
        if case == "no_writer":
            one[case] = None
            continue
        os.makedirs(os.path.join(tmp, case, "one"))
        ser = Simulation(copy.deepcopy(inp), base_dir=INPUTS, output_dir=os.path.join(tmp, case, "one"), **kw)
        ser.run()
        assert ser.ts.taken == STEPS
        one[case] = ser.datasets()
        ser.ode.destroy()
    world = 2
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, uid_q, q, tmp)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=280) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.exitcode is None:
                p.kill()
    assert [p.exitcode for p in procs] == [0] * world
    return {case: (one[case], [res[r][case] for r in range(world)]) for case in one}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", ["doublet", "minc", "reinjection"])
def test_gathered_datasets_are_the_one_rank_runs(runs, case):
    one, (root, other) = runs[case]
    got = root["data"]
    assert other["data"] is None and got is not None                   # rank 0 holds the snapshots, rank 1 none
    assert root["taken"] == other["taken"] == STEPS
    assert root["own_cells"] == root["n_owned"] and other["own_cells"] == other["n_owned"]      # run() still returns the rank's own cells
    assert sorted(got) == sorted(one), sorted(set(got) ^ set(one))
    for k in sorted(one):
        assert got[k].shape == one[k].shape and got[k].dtype == one[k].dtype, (k, got[k].shape, one[k].shape)
        assert not np.isnan(got[k]).any(), k                          # every place filled
        if k.startswith(EXACT):
            assert np.array_equal(got[k], one[k]), k
        else:
            sc = max(np.abs(one[k]).max(), 1e-300)
            err = np.abs(got[k] - one[k]).max() / sc
            print("  %-12s %-52s %.2e of its largest magnitude %.4g" % (case, k, err, sc))
            assert err <= TOL, (k, err)
    if case == "minc":
        assert "/minc/level" in got and got["/minc/level"].max() == 2
    if case == "doublet":
        assert got["/cell_fields/tracer_tracer1"].max() > 1e-6 and got["/source_fields/source_rate"].shape == (1, 2)
    if case == "reinjection":
        assert got["/time"].shape == (4, 1)                            # initial, steps 2 and 4, final
        for k in ("/face_fields/flux_water", "/face_fields/flux_energy", "/face_fields/flux_liquid", "/face_fields/flux_vapour",
                  "/source_fields/source_steam_rate", "/source_fields/network_group_rate", "/source_fields/network_reinject_output_water_rate",
                  "/face_cell_1", "/face_cell_2", "/face_fields/face_geometry_area"):
            assert k in got, k
        assert np.abs(got["/face_fields/flux_water"]).max() > 0 and got["/source_fields/network_group_rate"][-1, 0] < -1.0


@pytest.mark.parametrize("case", ["doublet", "minc", "reinjection"])
def test_the_root_writes_the_file_and_nobody_else(runs, case):
    if not _hdf5():
        pytest.skip("the HDF5 library does not load here: the file is not written (Simulation.output_error says so)")
    one, (root, other) = runs[case]
    name = _inputs()[case][0]["output"]["filename"]
    assert root["error"] is None and other["error"] is None
    assert root["files"] == [name] and other["files"] == []
    for k, v in root["data"].items():
        back = np.asarray(root["back"][k])
        assert back.shape == v.shape and np.array_equal(back, v), k


def test_without_the_hdf5_library_the_root_gathers_and_reports(runs):
    """the doublet once more with a writer that raises on rank 0 alone, as where its HDF5 library does not load: rank 0 took
    part in every gather all the same (the run ended, the snapshots are there and equal the run's that wrote), the failure is
    rank 0's output_error, and no file appears"""
    _, (root, other) = runs["no_writer"]
    _, (wrote, _) = runs["doublet"]
    assert root["taken"] == other["taken"] == STEPS
    assert root["error"] is not None and "no HDF5 library" in root["error"] and other["error"] is None
    assert root["files"] == [] and other["files"] == []
    assert sorted(root["data"]) == sorted(wrote["data"]) and all(np.array_equal(root["data"][k], wrote["data"][k]) for k in wrote["data"])


@pytest.mark.timeout(300)
def test_run_module_under_the_launcher_writes_one_file(tmp_path):
    """`python -m torch.distributed.run --nproc-per-node 2 -m waiwera_amd.run doublet.json`: the input's output file appears
    once, in the output directory, with the whole mesh's cells"""
    if not _hdf5():
        pytest.skip("the HDF5 library does not load here: no output file on any number of ranks")
    from waiwera_amd import hdf5io
    inp = _inputs()["doublet"][0]
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir(), dst.mkdir()
    for f in ("gdoublet.msh", "doublet_ss.h5"):
        shutil.copy(os.path.join(INPUTS, f), src / f)
    path = str(src / "doublet.json")
    json.dump(inp, open(path, "w"))
    env = dict(os.environ, WAI_RCCL_LIB=LOOPBACK, WAI_BENCH_LOOPBACK="1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT,
               WAIWERA_OUTPUT_DIR=str(dst))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "-m", "waiwera_amd.run", path]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "finished at t =" in r.stdout
    assert sorted(os.listdir(str(dst))) == ["doublet.h5"]
    assert sorted(os.listdir(str(src))) == ["doublet.json", "doublet_ss.h5", "gdoublet.msh"]
    p = hdf5io.read_dataset(str(dst / "doublet.h5"), "/cell_fields/fluid_pressure")
    assert p.shape == (1, 100) and np.isfinite(p).all()
