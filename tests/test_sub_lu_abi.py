"""The sub-preconditioner switch's entry point (wai_set_sub_pc: WAI_SUB_ILU | WAI_SUB_LU) at every layer a host reaches
it through: the C header, the Fortran module, the ctypes binding and the Python classes.  No GPU needed."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_switch():
    hdr = open(os.path.join(ROOT, "include", "waiwera_hip.h")).read()
    assert re.search(r"int\s+wai_set_sub_pc\s*\(\s*wai_ctx\s*\*\s*ctx\s*,\s*int\s+sub\s*\)\s*;", hdr)
    assert re.search(r"WAI_SUB_ILU\s*=\s*0\s*,\s*WAI_SUB_LU\s*=\s*1", hdr)


def test_fortran_module_has_the_interface_and_a_type_bound_procedure():
    text = open(os.path.join(ROOT, "waiwera_amd", "fortran", "waiwera_hip_module.F90")).read()
    assert 'bind(c, name = "wai_set_sub_pc")' in text
    assert re.search(r"procedure, public :: set_sub_pc => hip_sim_set_sub_pc", text)
    assert re.search(r"WAI_SUB_ILU = 0, WAI_SUB_LU = 1", text)


def test_python_binds_it_and_refuses_a_null_context():
    from waiwera_amd import lib
    from waiwera_amd.flow_simulation import FlowSimulation
    from waiwera_amd.simulation import Simulation
    assert lib.SUB_PC == {"ilu": 0, "lu": 1}
    assert lib.LIB.wai_set_sub_pc(None, 1) == -2      # a null context is refused, not dereferenced
    assert hasattr(FlowSimulation, "set_sub_pc")
    assert inspect.signature(Simulation.__init__).parameters["sub_lu"].default == "host"
