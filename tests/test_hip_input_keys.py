"""The input keys the device newly honours, on the device: thermodynamics.extrapolate (wai_set_thermo_extrapolate: region 1's
upper temperature bound 360 instead of 350 deg C) against numbers of the reference's own IAPWS.F90 / IFC67.F90
(tests/golden/reference_unit_values_extrapolate.json) and in a Newton step; source.production_component
(wai_set_source_production_component) against the definition restated in tests/source_component_reference.py, and through
the batched coupling build; mesh.permeability_angle through the face data the device already takes."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch.multiprocessing  # noqa: F401  (before the library, as tests/test_hip_coupling_batched.py has it: its DeviceVector
#                                     allocates through the copy of the HIP runtime the process mapped first)

import waiwera_amd.mesh as M
from tests import source_component_reference as ref
from tests.test_hip_coupling_batched import check_against_columns, context, first_cells
from tests.test_input_keys import base_input, write_2x2
from waiwera_amd import lib as wl
from waiwera_amd.cases import make_case, scaled

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LIQ = 7      # first field of the liquid phase in the fluid record of eos we: density, viscosity, ..., internal energy at + 6


def P(a):
    return a.ctypes.data_as(C.POINTER(C.c_int if a.dtype == np.int32 else C.c_double))


# ---- thermodynamics.extrapolate: known answers ----------------------------------------------------------------------------
with open(os.path.join(HERE, "golden", "reference_unit_values_extrapolate.json")) as _f:
    GOLD = json.load(_f)


def region1_state(sim, p, t):
    """(error flag, liquid density, internal energy, viscosity) of region 1 at (p, t) through the device EOS: cell 0 of a
    two-cell mesh, the other cell at a state every bound admits"""
    y = np.array([p / 1.0e6, t / 1.0e2, 0.1, 0.2])
    rc = sim.pre_eval(0.0, y)
    f = sim.fluid()[0]
    return (1 if rc > 0 else 0), f[LIQ], f[LIQ + 6], f[LIQ + 1]


@pytest.mark.parametrize("thermo", ["iapws", "ifc67"])
def test_region1_up_to_360_degrees_against_the_reference(thermo):
    """rho and u to 1e-7 relative, the tolerance tests/test_hip_ifc67.py holds the reference's unit values to; viscosity to
    1e-6 (tests/test_hip_salt.py).  The flags exactly: none up to 360 deg C, error 1 at 360.5, and error 1 from 350.5 deg C
    on with the setter off.  (30 MPa, 355 deg C) is the reference's own case, IFC67_test.F90:261-287"""
    from waiwera_amd.flow_simulation import FlowSimulation
    lm = M.StructuredGrid((2, 1, 1), brick=(2, 1, 1)).local_mesh(0)
    sim = FlowSimulation(lm, eos="we", thermo=thermo)
    sim.set_regions(np.ones(2, dtype=np.int32))
    cases = GOLD[thermo]
    assert {(c["p"], c["t"]) for c in cases} >= {(p, t) for p in (1.0e6, 20.0e6, 90.0e6) for t in (350.0, 350.5, 355.0, 360.0, 360.5)}
    assert any((c["p"], c["t"], c["err"], c["err_off"]) == (30.0e6, 355.0, 0, 1) for c in cases)
    assert not sim.thermo_extrapolate()
    off = [region1_state(sim, c["p"], c["t"])[0] for c in cases]
    sim.set_thermo_extrapolate(True)
    assert sim.thermo_extrapolate()
    on = [region1_state(sim, c["p"], c["t"]) for c in cases]
    sim.set_thermo_extrapolate(False)
    assert not sim.thermo_extrapolate()
    again = [region1_state(sim, c["p"], c["t"])[0] for c in cases]
    sim.destroy()
    for c, e_off, (e_on, rho, u, mu), e_again in zip(cases, off, on, again):
        print(thermo, c["p"], c["t"], "flags", e_off, e_on, "rho, u, mu", rho, u, mu)
        assert e_off == c["err_off"] == e_again, (c, e_off, e_again)
        assert e_on == c["err"], (c, e_on)
        if c["err"] == 0:
            assert abs(rho - c["rho"]) <= 1e-7 * c["rho"], (c, rho)
            assert abs(u - c["u"]) <= 1e-7 * c["u"], (c, u)
            assert abs(mu - c["viscosity"]) <= 1e-6 * c["viscosity"], (c, mu)
    assert sum(c["err"] == 0 and c["err_off"] == 1 for c in cases) >= 6      # states only the extrapolated bound admits


# ---- thermodynamics.extrapolate: in a run ------------------------------------------------------------------------------------
def heated_column(extrapolate):
    """a column of three 10 m cubes of the default rock at 30 MPa and 349 deg C, liquid; the middle cell takes heat for one
    step of 1e4 s.  Per m3 and K the rock holds 0.9 * 2200 * 1000 J and the water about 0.1 * 645 kg * 6.3e3 J/kg (du/dT of
    the golden values at 30 MPa), 2.4e6 J together: 1.43e6 W into 1000 m3 for 1e4 s is about + 6 K"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g = M.StructuredGrid((1, 1, 3), brick=(1, 1, 3))
    lm = g.local_mesh(0, sources=[{"ijk": (0, 0, 1), "rate": 1.43e6, "enthalpy": 0.0, "component": 2}])
    sim = FlowSimulation(lm, eos="we", thermo_extrapolate=extrapolate)
    region = np.ones(3, dtype=np.int32)
    sim.set_regions(region)
    y = np.tile([30.0, 3.49], 3).astype(np.float64)
    reason, nits, kits = sim.timestep(0.0, 1.0e4, y)
    heated = int(np.asarray(lm.src_cell)[0])
    sim.destroy()
    return reason, nits, 100.0 * y[2 * heated + 1]


def test_newton_step_into_the_extrapolated_range():
    reason, nits, t = heated_column(False)
    print("off: reason", reason, "its", nits, "T", t)
    assert reason < 0, "without the key a cell heated past 350 deg C is a domain error: the step fails and is retried"
    reason, nits, t = heated_column(True)
    print("on: reason", reason, "its", nits, "T", t)
    assert reason > 0 and 350.5 < t < 360.0, (reason, t)


# ---- source.production_component against the definition ------------------------------------------------------------------------
STATE = {"we": ([5.0e6, 0.3], 4), "wce": ([5.0e6, 0.3, 1.0e5], 4)}


def source_case(eos, c):
    """(cell, rate, enthalpy, component, production component): producing and injecting sources share cells 1 and 3"""
    np_ = ref.NP[eos]
    return [(1, -2.0, 0.0, 0, c), (1, 1.5, 5.0e5, 1, c), (2, -1.0, 0.0, 0, c), (2, -0.5, 0.0, 1, 0),
            (3, 2.0e4 if np_ == 2 else 0.25, 2.0e5, 2, c), (3, -0.75, 0.0, np_, c), (3, -0.125, 0.0, 0, 0)]


def rhs_with(eos, sources, production):
    """wai_rhs, the fluid record and the cell volumes of a row of four cells in one two-phase state: no gravity along the
    row and no gradient, so that the fluxes are zero and a row of wai_rhs is the source term alone.  production: None (the
    entry point is not called), "null" (called with NULL after the components were set) or the components"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, _, _ = make_case(dims=(4, 1, 1), brick=(4, 1, 1), eos=eos, sources=False, top_bc=False, hetero=False)
    sim = FlowSimulation(lm, eos=eos)
    prim, r = STATE[eos]
    region = np.full(4, r, dtype=np.int32)
    sim.set_regions(region)
    y = scaled(np.tile(prim, (4, 1)), region, eos).ravel().copy()
    keep = (wl._i32([s[0] for s in sources]), wl._f64([s[1] for s in sources]), wl._f64([s[2] for s in sources]),
            wl._i32([s[3] for s in sources]), wl._i32([s[4] for s in sources]))
    sim._chk(wl.LIB.wai_set_sources(sim.h, len(sources), P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3])), "set_sources")
    if production is not None:
        sim._chk(wl.LIB.wai_set_source_production_component(sim.h, P(keep[4])), "set_source_production_component")
    if production == "null":
        sim._chk(wl.LIB.wai_set_source_production_component(sim.h, None), "set_source_production_component")
    assert sim.pre_eval(0.0, y) == 0
    out = np.zeros(sim.num_dof)
    assert sim.rhs(0.0, (0.0, 0.0), y, out) == 0
    fluid = sim.fluid()[:4].copy()
    sim.destroy()
    return out.reshape(4, -1), fluid, np.asarray(lm.cell_geom)[:4, 3].copy()


@pytest.mark.parametrize("eos, c", [("we", 1), ("we", 2), ("wce", 2), ("wce", 3), ("we", 0), ("wce", 0)])
def test_source_term_with_a_production_component(eos, c):
    """every row of wai_rhs to 1e-14 relative: a handful of products formed the same way on both sides"""
    sources = source_case(eos, c)
    got, fluid, vol = rhs_with(eos, sources, "set")
    want = ref.source_rows(fluid, eos, vol, sources)
    print(eos, c, "got", got.tolist(), "want", want.tolist())
    assert np.all(got[0] == 0.0) and np.all(want[0] == 0.0), "a cell without sources: no gradient, no flux"
    assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want)), np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    if c > 0 and eos == "wce":
        # the whole rate in component c, none spread over water and gas by their flow fractions
        none, _, _ = rhs_with(eos, [s[:4] + (0,) for s in sources], None)
        assert not np.array_equal(got, none)


@pytest.mark.parametrize("eos", ["we", "wce"])
def test_no_production_component_is_the_result_as_before_bit_for_bit(eos):
    sources = source_case(eos, 0)
    never, fluid, vol = rhs_with(eos, sources, None)
    zeros, _, _ = rhs_with(eos, sources, "set")
    reset, _, _ = rhs_with(eos, source_case(eos, ref.NP[eos]), "null")
    assert never.tobytes() == zeros.tobytes() == reset.tobytes()
    want = ref.source_rows(fluid, eos, vol, sources)
    assert np.all(np.abs(never - want) <= 1e-14 * np.abs(want))


def test_heat_only_producer_reports_no_enthalpy_and_bad_components_are_refused():
    from waiwera_amd.flow_simulation import FlowSimulation, WaiError
    g = M.StructuredGrid((2, 1, 1), brick=(2, 1, 1))
    lm = g.local_mesh(0, sources=[{"ijk": (0, 0, 0), "rate": -1.0, "enthalpy": 0.0, "component": 0},
                                  {"ijk": (1, 0, 0), "rate": -1.0, "enthalpy": 0.0, "component": 0}])
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(np.ones(2, dtype=np.int32))
    y = np.array([5.0, 1.5, 5.0, 1.5])
    sim.set_source_production_component([2, 1])
    assert sim.pre_eval(0.0, y) == 0
    rate, enth = sim.source_rates()
    assert list(rate) == [-1.0, -1.0] and enth[0] == 0.0 and enth[1] > 6.0e5      # source.F90:419-425
    with pytest.raises(WaiError, match="production component"):
        sim.set_source_production_component([3, 0])
    with pytest.raises(ValueError):
        sim.set_source_production_component([1])
    sim.destroy()


def test_batched_coupling_build_with_production_components():
    """k_cb_raw restates k_source_rates: with production components set -- mass, heat alone, none -- the batched build's
    blocks are the column loop's, bit for bit (check_against_columns, tests/test_hip_coupling_batched.py)"""
    sim, lm, y, cells = context((4, 4, 2), "we", first_cells(4), lambda m: 8)
    pc = wl._i32([(1, 2, 0)[i % 3] if i % 4 != 3 else 0 for i in range(8)])
    sim._chk(wl.LIB.wai_set_source_production_component(sim.h, P(pc)), "set_source_production_component")
    with_pc = check_against_columns(sim, y, 4, 2).copy()
    sim._chk(wl.LIB.wai_set_source_production_component(sim.h, None), "set_source_production_component")
    without = check_against_columns(sim, y, 4, 2)
    assert not np.array_equal(with_pc, without), "the production components change the couplings"
    sim.destroy()


# ---- mesh.permeability_angle on the device -----------------------------------------------------------------------------------
def rhs_of_input(tmp_path, angle, permeability):
    from waiwera_amd.simulation import Simulation
    write_2x2(str(tmp_path / "m.msh"))
    inp = copy.deepcopy(base_input(permeability_angle=angle) if angle is not None else base_input())
    inp["rock"]["types"][0]["permeability"] = permeability
    inp["initial"] = {"primary": [[2.0e5, 20.0], [3.0e5, 25.0], [2.5e5, 30.0], [4.0e5, 22.0]], "region": 1}
    sim = Simulation(inp, base_dir=str(tmp_path))
    assert sim.ode.pre_eval(0.0, sim.y) == 0
    out = np.zeros(sim.ode.num_dof)
    assert sim.ode.rhs(0.0, (0.0, 0.0), sim.y, out) == 0
    sim.ode.destroy()
    return out


def test_anisotropic_rock_turned_by_90_degrees(tmp_path):
    """kx = 100 ky at 90 degrees gives the wai_rhs that angle 0 gives with kx and ky swapped, bit for bit"""
    turned = rhs_of_input(tmp_path, 90.0, [1.0e-13, 1.0e-15, 1.0e-14])
    swapped = rhs_of_input(tmp_path, 0.0, [1.0e-15, 1.0e-13, 1.0e-14])
    plain = rhs_of_input(tmp_path, None, [1.0e-13, 1.0e-15, 1.0e-14])
    assert np.abs(turned).max() > 0.0
    assert turned.tobytes() == swapped.tobytes()
    assert turned.tobytes() != plain.tobytes(), "the angle reaches the fluxes"
