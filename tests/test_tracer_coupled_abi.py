"""The coupled tracer solve's entry points (wai_set_tracer_solve_mode, wai_tracer_block_system; the sweep counter
wai_tracer_stats of the bench header) without a GPU: exported, declared to Fortran hosts, bound by waiwera_amd.lib with the
header's argument lists, reachable from the front end."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wai_set_tracer_solve_mode", "wai_tracer_block_system")


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_symbols_are_exported():
    from waiwera_amd import build
    lib = C.CDLL(build.build())
    for s in NEW + ("wai_tracer_stats",):
        assert hasattr(lib, s), s
    # a null context is refused, not dereferenced
    lib.wai_set_tracer_solve_mode.argtypes = [C.c_void_p, C.c_int]
    assert lib.wai_set_tracer_solve_mode(None, 1) == -2


def test_header_declares_the_modes():
    h = header("waiwera_hip.h")
    assert re.search(r"WAI_TRACER_PER_TRACER\s*=\s*0\s*,\s*WAI_TRACER_COUPLED\s*=\s*1", h)
    assert "wai_tracer_stats" in header("waiwera_hip_bench.h") and "wai_tracer_stats" not in h


def test_fortran_module_declares_them():
    text = open(os.path.join(ROOT, "waiwera_amd", "fortran", "waiwera_hip_module.F90")).read()
    joined = re.sub(r"&\s*\n", " ", text)
    for s in NEW:
        assert re.search(r'function\s+%s\(.*bind\(c,\s*name\s*=\s*"%s"\)' % (s, s), joined), s
        assert any(s in ln for ln in joined.splitlines() if ln.strip().startswith("public ::")), s


def c_args(decl):
    """ctypes classes of a C declaration's parameters"""
    out = []
    for a in decl.split(","):
        a = a.strip()
        if "*" in a:
            out.append("ptr")
        elif a.startswith("double"):
            out.append("double")
        else:
            out.append("int")
    return out


def test_python_prototypes_match_the_header():
    from waiwera_amd import lib
    text = header("waiwera_hip.h") + header("waiwera_hip_bench.h")
    for s in NEW + ("wai_tracer_stats",):
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % s, text)
        assert m, s
        want = c_args(m.group(1))
        fn = getattr(lib.LIB, s)
        got = ["double" if a is C.c_double else "int" if a is C.c_int else "ptr" for a in fn.argtypes]
        assert got == want, (s, got, want)
        assert fn.restype is C.c_int
    assert lib.TRACER_SOLVE == {"per_tracer": 0, "coupled": 1}


def test_front_end_takes_the_switch():
    import inspect
    from waiwera_amd import run
    from waiwera_amd.flow_simulation import FlowSimulation
    from waiwera_amd.simulation import Simulation
    from waiwera_amd.timestepper import Timestepper
    assert inspect.signature(Simulation.__init__).parameters["tracer_solve"].default == "per_tracer"
    assert inspect.signature(Timestepper.__init__).parameters["tracer_solve_mode"].default is None
    assert hasattr(FlowSimulation, "set_tracer_solve_mode") and hasattr(FlowSimulation, "aux_block_system")
    assert "--tracer-solve" in inspect.getsource(run.main)
    # the reference's input schema has no such key: the front end reads none
    src = inspect.getsource(Simulation)
    assert not re.search(r"""(inp|step|_get)\W.*tracer_solve""", src.replace("self.tracer_solve", ""))
