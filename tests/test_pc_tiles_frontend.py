"""wai_set_pc_tiles at every layer a host reaches it through without a device: the C header, the Fortran module, the ctypes
binding, the Python classes and the command line; and what the input front end hands the flow object under
subdomains="rank" -- one block per rank with the chunks it builds today as tiles -- on one rank and on two, with the flow
object replaced by the recording stub of tests/test_input_partition.py (imported)."""
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_input_partition import COLLECTIVE, RecordingOde, _load, _sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_at_every_layer():
    hdr = open(os.path.join(ROOT, "include", "waiwera_hip.h")).read()
    assert re.search(r"int\s+wai_set_pc_tiles\s*\(\s*wai_ctx\s*\*\s*ctx\s*,\s*int\s+n_tiles\s*,\s*const\s+int\s*\*\s*tile_ptr\s*\)\s*;", hdr)
    bench = open(os.path.join(ROOT, "include", "waiwera_hip_bench.h")).read()
    assert re.search(r"int\s+wai_test_tile_schedule\s*\(", bench) and "wai_test_tile_schedule" not in hdr
    f90 = open(os.path.join(ROOT, "waiwera_amd", "fortran", "waiwera_hip_module.F90")).read()
    assert 'bind(c, name = "wai_set_pc_tiles")' in f90
    assert re.search(r"procedure, public :: set_pc_tiles => hip_sim_set_pc_tiles", f90)
    from waiwera_amd import lib
    from waiwera_amd.flow_simulation import FlowSimulation
    from waiwera_amd.simulation import Simulation
    assert lib.LIB.wai_set_pc_tiles(None, 0, None) == -2      # a null context is refused, not dereferenced
    assert hasattr(FlowSimulation, "set_pc_tiles") and hasattr(FlowSimulation, "tile_schedule")
    assert inspect.signature(Simulation.__init__).parameters["subdomains"].default == "chunks"
    run = open(os.path.join(ROOT, "waiwera_amd", "run.py")).read()
    assert '"--subdomains", choices=("chunks", "rank"), default="chunks"' in run


@pytest.mark.parametrize("world", [1, 2])
def test_subdomains_rank_hands_the_chunks_over_as_tiles(world):
    """problem 5a: under "rank" the context is created with sub_ptr = None and set_pc_tiles gets the chunk list that "chunks"
    -- the default, unchanged -- creates the context with; on two ranks each rank's own chunks"""
    inp = _load("problem5a.json")
    for rank in range(world):
        RecordingOde.made.clear()
        a = _sim(inp, rank, world)
        (ode_a,) = RecordingOde.made
        chunks = np.asarray(a.mesh.sub_ptr).copy()
        assert chunks[0] == 0 and chunks[-1] == a.mesh.n_owned and not ode_a.named("set_pc_tiles")
        assert a.subdomain_choice[0] == "chunks"
        RecordingOde.made.clear()
        b = _sim(inp, rank, world, subdomains="rank")
        (ode_b,) = RecordingOde.made
        assert ode_b.mesh.sub_ptr is None and b.mesh.n_owned == a.mesh.n_owned
        ((name, args, kw),) = ode_b.named("set_pc_tiles")
        assert np.array_equal(args[0], chunks) and not kw
        assert b.subdomain_choice[0] == "rank" and "%d chunks" % (chunks.size - 1) in b.subdomain_choice[1]
        names = [c[0] for c in ode_b.calls]
        assert not COLLECTIVE & set(names[:names.index("set_pc_tiles")])
        assert b.pc_choice == a.pc_choice


def test_an_unknown_value_is_refused_before_the_flow_object_exists():
    inp = _load("problem5a.json")
    for world, ranks in ((1, [0]), (2, [0, 1])):
        for rank in ranks:
            RecordingOde.made.clear()
            with pytest.raises(ValueError, match="subdomains 'chunks'"):
                _sim(inp, rank, world, subdomains="bricks")
            assert not RecordingOde.made
