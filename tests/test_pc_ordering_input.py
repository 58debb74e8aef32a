"""The front end's side of the multicolour ordering without a GPU: what pc_ordering="multicolour" does not combine with is
decided from the input's solver object and the arguments alone (simulation.pc_ordering_refusal), so every rank decides alike;
the binding's table and the C header agree."""
import os
import re

import pytest

from waiwera_amd import lib
from waiwera_amd.simulation import Simulation, linear_solver_options, pc_ordering_refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lso(pc=None, sub=None, levels=None, default_pc="bjacobi", sub_lu="host"):
    obj = {}
    if pc:
        obj["preconditioner"] = {"type": pc}
    if sub or levels is not None:
        s = {"type": sub or "ilu"}
        if levels is not None:
            s["factor"] = {"levels": levels}
        obj.setdefault("preconditioner", {})["sub"] = {"preconditioner": s}
    return linear_solver_options(obj, default_pc, sub_lu)


def test_served_combinations():
    assert pc_ordering_refusal(lso("bjacobi"), False) is None
    assert pc_ordering_refusal(lso("ilu"), False) is None              # the one-block case of bjacobi
    assert pc_ordering_refusal(lso(None, default_pc="bjacobi"), False) is None
    assert pc_ordering_refusal(lso("bjacobi", levels=0), False) is None
    # ignored, as in the library: no preconditioner, and the dense block inverses sub lu maps to by default
    assert pc_ordering_refusal(lso("none"), True) is None
    assert pc_ordering_refusal(lso("lu"), False) is None
    assert pc_ordering_refusal(lso("bjacobi", sub="lu"), False) is None


@pytest.mark.parametrize("options,network,party", [
    (dict(pc="asm"), False, "asm"),
    (dict(pc=None, default_pc="asm"), False, "asm"),                   # the reference's default for an input that names none
    (dict(pc="bjacobi", levels=2), False, "factor.levels 2"),
    (dict(pc="bjacobi", sub="lu", sub_lu="device"), False, "sub-preconditioner lu"),
    (dict(pc="bjacobi"), True, "source network"),
])
def test_refused_combinations(options, network, party):
    msg = pc_ordering_refusal(lso(**options), network)
    assert msg is not None and "pc_ordering 'multicolour'" in msg and party in msg, msg


def test_unknown_ordering_is_a_value_error():
    with pytest.raises(ValueError, match="pc_ordering"):
        Simulation({}, pc_ordering="red-black")


def test_binding_table_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "waiwera_hip.h")).read()
    m = re.search(r"enum \{ WAI_PC_ORDER_NATURAL = (\d+), WAI_PC_ORDER_MULTICOLOUR = (\d+) \};", hdr)
    assert m and lib.PC_ORDER == {"natural": int(m.group(1)), "multicolour": int(m.group(2))}
    f90 = open(os.path.join(ROOT, "waiwera_amd", "fortran", "waiwera_hip_module.F90")).read()
    assert re.search(r"WAI_PC_ORDER_NATURAL = %s, WAI_PC_ORDER_MULTICOLOUR = %s" % m.groups(), f90)


def test_command_line_has_the_switch(capsys):
    from waiwera_amd import run
    with pytest.raises(SystemExit):
        run.main(["--help"])
    assert "--pc-ordering" in capsys.readouterr().out
