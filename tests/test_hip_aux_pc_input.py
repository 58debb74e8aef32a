"""The input front end's auxiliary solver object ("time.step.solver.auxiliary") on the GPU: tracer/oned (two-phase) with its
tracer entered twice, solved coupled under the reference's defaults -- the flow solver under asm, the tracers under block
Jacobi -- against the benchmark's AUTOUGH2 table at the 1e-3 / 1e-4 of tests/test_hip_input.py."""
import json
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")


@pytest.fixture(scope="module")
def two_tracers(tmp_path_factory):
    d = tmp_path_factory.mktemp("aux_pc")
    for f in ("oned_two_phase.json", "oned_two_phase_ss.h5", "goned.msh"):
        shutil.copy(os.path.join(INPUTS, f), d / f)
    inp = json.load(open(d / "oned_two_phase.json"))
    inp["tracer"] = [{"name": "first"}, {"name": "second"}]
    return inp, str(d)


def run_and_check(sim):
    from tests import benchmarks as B
    assert sim.pc_choice[0] == "asm" and sim.aux_pc_choice[0] == "bjacobi"
    assert sim.ode.get_aux_pc() == dict(pc_type="bjacobi", asm_overlap=1, ilu_levels=0, sub_pc="ilu")
    s0 = sim.ode.tracer_assembly_sweeps()
    out = sim.run()
    assert sim.ode.tracer_assembly_sweeps() - s0 == len(sim.ts.aux_history) > 0    # one sweep per step: the coupled path ran
    a = B.load_tracer_oned()["cases"]["two"]["autough2_final_table"]
    Xa = np.asarray(a["Tracer/liquid"])
    for name in ("first", "second"):
        eX = np.abs(out["tracer_" + name] - Xa)
        print(name, "worst relative", (eX / np.maximum(Xa, 1e-300))[eX > 1.0e-4].max(initial=0.0), "worst absolute", eX.max())
        assert np.all((eX <= 1.0e-3 * Xa) | (eX <= 1.0e-4)), name
    assert (np.abs(out["fluid_pressure"] - a["Pressure"]) / np.asarray(a["Pressure"])).max() < 1.0e-3
    return out


def test_auxiliary_object_sets_the_tracer_solver(two_tracers):
    """an input that names bjacobi for the auxiliary solver and nothing for the flow solver sets up coupled with no
    default_pc: flow asm (the reference's default), tracers block Jacobi"""
    from waiwera_amd.simulation import Simulation
    inp, base = two_tracers
    inp = json.loads(json.dumps(inp))
    inp["time"]["step"].setdefault("solver", {})["auxiliary"] = {"preconditioner": {"type": "bjacobi"}}
    sim = Simulation(inp, base_dir=base, tracer_solve="coupled")
    assert sim.pc_choice[:2] == ("asm", "reference default") and sim.aux_pc_choice[:2] == ("bjacobi", "input")
    out = run_and_check(sim)
    sim.ode.destroy()
    # the same input without the object, the reference's auxiliary preconditioner asked for by argument: the same result
    inp2, _ = two_tracers
    sim = Simulation(json.loads(json.dumps(inp2)), base_dir=base, tracer_solve="coupled", default_aux_pc="bjacobi")
    assert sim.aux_pc_choice[:2] == ("bjacobi", "reference default")
    out2 = run_and_check(sim)
    sim.ode.destroy()
    for k in ("tracer_first", "tracer_second", "fluid_pressure"):
        assert np.array_equal(out[k], out2[k]), k


def test_an_input_that_follows_is_refused_as_before(two_tracers):
    """no auxiliary object, no default_aux_pc: the tracer solves follow the flow solver's asm, which the coupled mode does
    not cover -- the refusal and its text are the earlier ones; an uncovered auxiliary choice is refused by its own name"""
    from waiwera_amd.simulation import Simulation
    inp, base = two_tracers
    with pytest.raises(ValueError, match="default_pc='bjacobi'"):
        Simulation(json.loads(json.dumps(inp)), base_dir=base, tracer_solve="coupled")
    bad = json.loads(json.dumps(inp))
    bad["time"]["step"].setdefault("solver", {})["auxiliary"] = {"preconditioner": {"type": "asm"}}
    with pytest.raises(ValueError, match="auxiliary preconditioner is 'asm'"):
        Simulation(bad, base_dir=base, tracer_solve="coupled", default_pc="bjacobi")
    with pytest.raises(ValueError, match="default_aux_pc"):
        Simulation(json.loads(json.dumps(inp)), base_dir=base, default_aux_pc="ilu")
    # per tracer the follower runs, and says that it follows
    sim = Simulation(json.loads(json.dumps(inp)), base_dir=base)
    assert sim.aux_pc_choice[0] == "follow" and sim.ode.get_aux_pc()["pc_type"] == "follow"
    sim.ode.destroy()
