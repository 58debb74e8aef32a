"""waiwera_amd.simulation.linear_solver_options: one linear-solver object of the input ("time.step.solver.linear" or
"time.step.solver.auxiliary", the same keys: src/timestepper.F90:1645-1836, 2057-2065) -> the library's options.  Pure: no
library, no device.  The expected dictionaries are written out here, not taken from any code."""
import glob
import json
import os

import pytest

from waiwera_amd.simulation import AUXILIARY_DEFAULT_PC, AUXILIARY_DEFAULTS, covers_coupled, linear_solver_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")

# what the front end made of every golden input's "linear" object before the translation was a function of its own:
# (options handed to set_opts, sub-preconditioner lu on the device, pc_choice).  An input that is not listed has no object
LINEAR_EXPECTED = {
    "co2_column_1.json": ({"ksp_type": "bcgs", "pc_type": "bjacobi", "ilu_levels": 0}, False, ("bjacobi", "input")),
    "salt_column.json": ({"ksp_type": "bcgs", "pc_type": "asm", "ilu_levels": 0}, False, ("asm", "input")),
}
NO_OBJECT = ({"pc_type": "asm", "ilu_levels": 0}, False, ("asm", "reference default"))


def aux(obj, default_pc=AUXILIARY_DEFAULT_PC, sub_lu="host"):
    return linear_solver_options(obj, default_pc, sub_lu, AUXILIARY_DEFAULTS)


def test_module_needs_no_library():
    """the translation is importable and callable with the HIP library's binding never loaded"""
    import subprocess
    import sys
    code = ("import sys; from waiwera_amd.simulation import linear_solver_options as f; "
            "print(f({}, 'asm')['opts']['pc_type']); assert 'waiwera_amd.lib' not in sys.modules")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "asm", out.stderr


def test_empty_auxiliary_object_takes_the_reference_defaults():
    """gmres, rtol 1e-5, bjacobi over ILU(0) (default_auxiliary_ksp_type_str / default_auxiliary_pc_type_str,
    src/timestepper.F90:2021-2022)"""
    for obj in ({}, None):
        r = aux(obj)
        assert r["opts"] == {"ksp_type": "gmres", "ksp_rtol": 1e-5, "pc_type": "bjacobi", "ilu_levels": 0}
        assert (r["pc"], r["named"], r["sub_device"], r["note"]) == ("bjacobi", False, False, ())
        assert covers_coupled(r)
    assert (AUXILIARY_DEFAULTS, AUXILIARY_DEFAULT_PC) == ({"ksp_type": "gmres", "ksp_rtol": 1e-5}, "bjacobi")


def test_each_key_is_carried_through():
    obj = {"type": "lgmres", "tolerance": {"relative": 1e-9}, "maximum": {"iterations": 77},
           "options": {"gmres": {"restart": 12}},
           "preconditioner": {"type": "asm", "sub": {"preconditioner": {"type": "ilu", "factor": {"levels": 2}}}}}
    want = {"ksp_type": "lgmres", "ksp_rtol": 1e-9, "ksp_max_its": 77, "gmres_restart": 12, "pc_type": "asm", "ilu_levels": 2}
    for r in (aux(obj), linear_solver_options(obj, "bjacobi")):
        assert r["opts"] == want
        assert (r["pc"], r["named"], r["sub_device"]) == ("asm", True, False)
        assert not covers_coupled(r)
    for t in ("bcgs", "gmres", "bcgsl", "lgmres"):
        assert aux({"type": t})["opts"]["ksp_type"] == t
    # one key at a time beside the defaults
    assert aux({"tolerance": {"relative": 1e-8}})["opts"] == {"ksp_type": "gmres", "ksp_rtol": 1e-8, "pc_type": "bjacobi", "ilu_levels": 0}
    assert aux({"preconditioner": {"type": "none"}})["opts"]["pc_type"] == "none"
    assert aux({"preconditioner": {"type": "ilu"}})["opts"]["pc_type"] == "bjacobi"     # a serial run's "ilu": one block of bjacobi
    assert aux({"preconditioner": {"type": "ilu"}})["pc"] == "ilu"
    assert aux({}, default_pc="asm")["opts"]["pc_type"] == "asm" and not aux({}, default_pc="asm")["named"]
    # without defaults only what the object names is set (the flow solver: the library's own defaults stand)
    assert linear_solver_options({"type": "gmres"}, "asm")["opts"] == {"ksp_type": "gmres", "pc_type": "asm", "ilu_levels": 0}


def test_sub_preconditioner_lu_mappings():
    sub = {"sub": {"preconditioner": {"type": "lu"}}}
    r = aux({"preconditioner": dict(sub, type="asm")})
    assert r["opts"]["pc_type"] == "lu" and "ilu_levels" not in r["opts"] and not r["sub_device"]
    assert r["note"] == ("sub lu: dense block inverses from the host, block Jacobi (the overlap is dropped)",)
    r = aux({"preconditioner": sub})
    assert r["opts"]["pc_type"] == "lu" and r["note"] == ("sub lu: dense block inverses from the host, block Jacobi",)
    r = aux({"preconditioner": dict(sub, type="asm")}, sub_lu="device")
    assert r["opts"]["pc_type"] == "asm" and r["sub_device"] and not covers_coupled(r)
    assert r["note"] == ("sub lu: exact block solves on the device (wai_set_sub_pc)",)


@pytest.mark.parametrize("obj", [{"type": "cg"}, {"preconditioner": {"type": "gamg"}},
                                 {"preconditioner": {"sub": {"preconditioner": {"type": "cholesky"}}}},
                                 {"preconditioner": {"type": "none", "sub": {"preconditioner": {"factor": {"levels": 1}}}}}])
def test_unknown_types_raise(obj):
    with pytest.raises(NotImplementedError):
        aux(obj)
    with pytest.raises(NotImplementedError):
        linear_solver_options(obj, "asm")


def test_linear_objects_of_the_golden_inputs_translate_as_before():
    files = sorted(glob.glob(os.path.join(INPUTS, "*.json")))
    assert len(files) >= 20
    seen = set()
    for f in files:
        inp = json.load(open(f))
        obj = (((inp.get("time") or {}).get("step") or {}).get("solver") or {}).get("linear")
        name = os.path.basename(f)
        want = LINEAR_EXPECTED.get(name, NO_OBJECT)
        assert (obj is not None) == (name in LINEAR_EXPECTED), name
        seen.add(name)
        r = linear_solver_options(obj, "asm", "host")
        why = "input" if r["named"] else "reference default"
        assert (r["opts"], r["sub_device"], (r["pc"], why) + r["note"]) == want, name
        # ... and under the library's fast path as the default: only an input that names no preconditioner moves
        r = linear_solver_options(obj, "bjacobi", "host")
        assert r["opts"]["pc_type"] == ("bjacobi" if name not in LINEAR_EXPECTED else want[0]["pc_type"]), name
    assert set(LINEAR_EXPECTED) <= seen
