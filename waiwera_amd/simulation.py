"""Runs a simulation described by a Waiwera JSON input file (the subset the hot path covers) on the
HIP library: the reference's own input format on one side of the path, its output field names on
the other.

Input keys handled, with the reference's defaults (src/flow_simulation.F90:296-670, 800-846;
src/mesh.F90:270-300, 1640-1800; src/rock_setup.F90; src/initial.F90:421-677; src/source_setup.F90;
src/timestepper.F90:1960-2275; src/tracer.F90:63-140; utils/input_schema.json):

  mesh        filename (gmsh MSH 2.2), thickness, radial, zones (all / box ranges on x, y, z), permeability_angle,
              faces [cells, permeability_direction]
  gravity     number | vector | null
  eos         name w | we | wce | wae | wse | wsce | wsae, temperature, permeability_modifier
  thermodynamics  iapws | ifc67, or {name, extrapolate}
  rock        types [cells | zones, permeability, porosity, density, specific_heat, wet / dry
              conductivity], relative_permeability, capillary_pressure
  initial     primary (one record or one per cell), region (one or per cell), tracer; or
              filename + index: restart from a Waiwera HDF5 output file
  boundaries  primary, region, faces {cells, normal} (one or a list), tracer
  mesh        filename (gmsh 2.2 ASCII; or mesh_file=: a MULgraph geometry file), thickness, radial,
              zones (boxes, cell lists), minc {geometry, rock {fracture, matrix, zones | types}}
  source      cell, rate, enthalpy, tracer (constants or [[t, v], ...] tables with "interpolation":
              linear|step and "averaging": integrate|endpoint), component, production_component (integers or the
              component's name; "energy": the heat equation), deliverability {productivity,
              pressure}, recharge | injectivity {coefficient, pressure}, limiter {type, limit,
              separator_pressure}, separator {pressure}, direction, factor
  time        start, stop, step {size, adapt, maximum, method, solver.nonlinear, solver.linear, solver.auxiliary}
  tracer      name, phase, decay, activation, diffusion

  output      filename, initial, final, frequency, checkpoint {time, tolerance} (cell fields, source
              rate and enthalpy)

Every key of the reference's schema stands in KEY_TABLE below as handled, without effect on the numbers (title, logfile.*,
output.flush, mesh.rebalance) or refused with the reason (REFUSED_KEYS: eos.primary.scale.*, initial.minc, zones made of other
zones or by radius, mesh.minc.rock.cells, output.checkpoint.step, output.jacobian, source.cells / zones, source.rate.time /
enthalpy.time, reference pressure against enthalpy under recharge / injectivity, source.tracer.<name>,
time.step.solver.nonlinear.jacobian.differencing.* and tolerance.update.*, time.step.stop.size.*).  check_input_keys walks
the input before anything is read or built and raises NotImplementedError with the full path for a refused key and for a key
the schema does not have; values a handled key can carry but this front end does not cover are refused where they are read.

Sub-preconditioner "lu" ("preconditioner": {"sub": {"preconditioner": {"type": "lu"}}}) under bjacobi or asm has two
mappings.  The default (sub_lu="host") takes the library's pc_type "lu": dense block inverses formed on the host, block
Jacobi -- under "asm" this DROPS the overlap, a deviation from the reference -- and at most 8192 unknowns per block.
sub_lu="device" (python -m waiwera_amd.run --sub-lu device) keeps the outer preconditioner and sets the library's
sub-preconditioner lu (wai_set_sub_pc): bjacobi + exact block solves, or asm (overlap 1, PETSc's default: the input format has no key for it) +
exact local solves, which is the reference's meaning; factored and applied on the device.  pc_choice records the mapping taken.

The tracer solver reads "time.step.solver.auxiliary" (the keys of "linear").  What the object leaves out takes the
reference's auxiliary defaults: gmres, rtol 1e-5, bjacobi.  An input WITHOUT the object differs from the reference: its
tracer solves use the flow solver's preconditioner (asm for an unmodified input), not bjacobi; default_aux_pc="bjacobi"
(python -m waiwera_amd.run --aux-pc bjacobi) gives the reference's.  aux_pc_choice records what was taken.

Output: `Simulation.run` returns the final cell
fields under the reference's HDF5 dataset names (fluid_pressure, ...) and writes "output.filename"
in the reference's HDF5 layout (waiwera_amd/hdf5io.py, HDF5 C library through ctypes); `save`
writes a .npz archive.

N ranks (rank, world, comm_id; one process per rank, python -m waiwera_amd.run under a launcher): every rank reads the
whole input, builds the whole mesh -- MINC cells included -- and keeps its cells with one ghost layer
(waiwera_amd/partition.py).  Covered: everything above -- sources with their tables and
state-dependent controls, MINC zones (a family never leaves its fracture cell's rank), rock table controls (each rank
updates the controlled cells it holds, ghosts included), tracers in both solve modes (boundary values through the rank's
boundary cells, injection through its sources) and source networks (every rank holds the whole network, its sources
numbered as in the input; the library gathers their rates).  fields() returns the rank's cells, owned_gid their numbers
in the one-rank output (the input's numbering; a MINC mesh: the reference's cell order), source fields the rank's own
sources with owned_source their numbers in the input, group and reinjector fields the same on every rank.
"output.filename" on N ranks: every snapshot is gathered to rank 0 through the library (_gathered_fields: wai_gather_fluid
for the fluid record's columns, wai_gather_rows for geometry, tracers, source and flux fields), rank 0 writes the file a
one-rank run writes and carries output_error; save() / python -m waiwera_amd.run -o still write one .npz per rank.  NOT on
N ranks: PCASM overlap deeper than 1, which the library refuses.
Cell order (cell_order="compact", python -m waiwera_amd.run --cell-order compact; subdomain_rows / --subdomain-rows the cap):
the library gets the mesh numbered by wai_cell_order -- compact 3-D preconditioner subdomains numbered inside like bricks --
instead of the mesh file's numbering in chunks of consecutive cells.  Every cell number of the input (boundaries, sources,
rock types, zones given as cell lists, per-cell initial conditions, a restart file's cells) goes in through the inverse
permutation, and fields(), datasets(), the HDF5 file, save() and face_cell_1 / face_cell_2 come back in the input's numbering;
cell_order_choice records the order, the subdomains and the share of interior faces they cut.  One rank, a mesh file and no
MINC zones: the rest is refused by name (ValueError) from the input and the arguments alone.
Collective-call discipline: nothing that exchanges data stands under a condition that can differ
between ranks; what must be refused is refused from the input and the arguments alone, so on every rank alike.
"""
import collections
import json
import os

import numpy as np

from . import gmsh, unstructured
from .timestepper import Timestepper
from .interpolation import Table

UNSUPPORTED_SOURCE_KEYS = ()


def _get(d, path, default=None):
    for k in path.split("."):
        if not isinstance(d, dict) or k not in d or d[k] is None:
            return default
        d = d[k]
    return d


# ---- every key of an input file: honoured, without effect on the numbers, or refused by name ---------------------------
# One entry per key path of the reference's schema (utils/input_schema.json; tests/golden/input_schema_paths.txt lists them).
# Normal form of a path: keys joined by dots, an array's elements under the array's own path (source[2].rate and a single
# tracer object's tracer.name alike: "source.rate", "tracer.name"), "*" for a name the user chooses (zones, tracers).
# HANDLED: read by this front end (which may still refuse a VALUE it does not cover, by name, where it reads it).
# NO_EFFECT: changes no computed number -- titles, the log, flushing, load balancing.
# REFUSED: would change the results or the files written and nothing here reads it.
HANDLED_KEYS = """
boundaries boundaries.faces boundaries.faces.cells boundaries.faces.normal boundaries.primary boundaries.region boundaries.tracer
eos eos.name eos.temperature eos.permeability_modifier eos.permeability_modifier.exponent eos.permeability_modifier.gamma
eos.permeability_modifier.phir eos.permeability_modifier.type eos.primary eos.primary.scale
gravity initial initial.filename initial.index initial.primary initial.region initial.tracer
mesh mesh.filename mesh.radial mesh.thickness mesh.permeability_angle mesh.faces mesh.faces.cells mesh.faces.permeability_direction
mesh.zones mesh.zones.* mesh.zones.*.cells mesh.zones.*.type mesh.zones.*.x mesh.zones.*.y mesh.zones.*.z
mesh.minc mesh.minc.geometry mesh.minc.geometry.fracture mesh.minc.geometry.fracture.connection
mesh.minc.geometry.fracture.planes mesh.minc.geometry.fracture.spacing mesh.minc.geometry.fracture.volume
mesh.minc.geometry.matrix mesh.minc.geometry.matrix.volume mesh.minc.rock mesh.minc.rock.fracture mesh.minc.rock.fracture.type
mesh.minc.rock.matrix mesh.minc.rock.matrix.type mesh.minc.rock.types mesh.minc.rock.zones
network network.group network.group.in network.group.limiter network.group.limiter.averaging
network.group.limiter.interpolation network.group.limiter.limit network.group.limiter.steam network.group.limiter.total
network.group.limiter.type network.group.limiter.water network.group.name network.group.scaling network.group.separator
network.group.separator.pressure network.reinject network.reinject.in network.reinject.name network.reinject.overflow
network.reinject.overflow.out network.reinject.steam network.reinject.steam.averaging network.reinject.steam.enthalpy
network.reinject.steam.interpolation network.reinject.steam.out network.reinject.steam.proportion network.reinject.steam.rate
network.reinject.water network.reinject.water.averaging network.reinject.water.enthalpy network.reinject.water.interpolation
network.reinject.water.out network.reinject.water.proportion network.reinject.water.rate
output output.checkpoint output.checkpoint.repeat output.checkpoint.time output.checkpoint.tolerance output.fields
output.fields.cell_geometry output.fields.face_geometry output.fields.fluid output.fields.flux output.fields.network_group
output.fields.network_reinject output.fields.source output.filename output.final output.frequency output.initial
rock rock.capillary_pressure rock.capillary_pressure.P0 rock.capillary_pressure.Pmax rock.capillary_pressure.interpolation
rock.capillary_pressure.lambda rock.capillary_pressure.pressure rock.capillary_pressure.saturation_limits
rock.capillary_pressure.slr rock.capillary_pressure.sls rock.capillary_pressure.type rock.relative_permeability
rock.relative_permeability.interpolation rock.relative_permeability.lambda rock.relative_permeability.liquid
rock.relative_permeability.power rock.relative_permeability.slr rock.relative_permeability.sls rock.relative_permeability.ssr
rock.relative_permeability.sum_unity rock.relative_permeability.type rock.relative_permeability.vapour
rock.types rock.types.cells rock.types.density rock.types.dry_conductivity rock.types.interpolation rock.types.name
rock.types.permeability rock.types.porosity rock.types.specific_heat rock.types.wet_conductivity rock.types.zones
source source.averaging source.cell source.component source.production_component source.deliverability
source.deliverability.pressure source.deliverability.pressure.enthalpy source.deliverability.pressure.pressure
source.deliverability.pressure.time source.deliverability.productivity source.deliverability.productivity.time
source.deliverability.threshold source.direction source.enthalpy source.factor source.factor.averaging
source.factor.interpolation source.factor.time source.injectivity source.injectivity.coefficient
source.injectivity.coefficient.time source.injectivity.pressure source.injectivity.pressure.time source.interpolation
source.limiter source.limiter.averaging source.limiter.interpolation source.limiter.limit source.limiter.separator_pressure
source.limiter.steam source.limiter.total source.limiter.type source.limiter.water source.name source.rate source.recharge
source.recharge.coefficient source.recharge.coefficient.time source.recharge.pressure source.recharge.pressure.time
source.separator source.separator.pressure source.tracer
thermodynamics thermodynamics.name thermodynamics.extrapolate
time time.start time.stop time.step time.step.adapt time.step.adapt.amplification time.step.adapt.maximum
time.step.adapt.method time.step.adapt.minimum time.step.adapt.on time.step.adapt.reduction time.step.maximum
time.step.maximum.number time.step.maximum.size time.step.maximum.tries time.step.method time.step.size time.step.solver
time.step.solver.auxiliary time.step.solver.auxiliary.maximum time.step.solver.auxiliary.maximum.iterations
time.step.solver.auxiliary.options time.step.solver.auxiliary.options.gmres time.step.solver.auxiliary.options.gmres.restart
time.step.solver.auxiliary.preconditioner time.step.solver.auxiliary.preconditioner.sub
time.step.solver.auxiliary.preconditioner.sub.preconditioner time.step.solver.auxiliary.preconditioner.sub.preconditioner.factor
time.step.solver.auxiliary.preconditioner.sub.preconditioner.factor.levels
time.step.solver.auxiliary.preconditioner.sub.preconditioner.type time.step.solver.auxiliary.preconditioner.type
time.step.solver.auxiliary.tolerance time.step.solver.auxiliary.tolerance.relative time.step.solver.auxiliary.type
time.step.solver.linear time.step.solver.linear.maximum time.step.solver.linear.maximum.iterations
time.step.solver.linear.options time.step.solver.linear.options.gmres time.step.solver.linear.options.gmres.restart
time.step.solver.linear.preconditioner time.step.solver.linear.preconditioner.sub
time.step.solver.linear.preconditioner.sub.preconditioner time.step.solver.linear.preconditioner.sub.preconditioner.factor
time.step.solver.linear.preconditioner.sub.preconditioner.factor.levels
time.step.solver.linear.preconditioner.sub.preconditioner.type time.step.solver.linear.preconditioner.type
time.step.solver.linear.tolerance time.step.solver.linear.tolerance.relative time.step.solver.linear.type
time.step.solver.nonlinear time.step.solver.nonlinear.maximum time.step.solver.nonlinear.maximum.iterations
time.step.solver.nonlinear.minimum time.step.solver.nonlinear.minimum.iterations time.step.solver.nonlinear.tolerance
time.step.solver.nonlinear.tolerance.function time.step.solver.nonlinear.tolerance.function.absolute
time.step.solver.nonlinear.tolerance.function.relative
tracer tracer.activation tracer.decay tracer.diffusion tracer.name tracer.phase
"""
NO_EFFECT_KEYS = """
title logfile logfile.echo logfile.filename logfile.format logfile.format.max_num_length logfile.format.num_real_digits
output.flush mesh.rebalance
"""
# why each is refused, for the message
REFUSED_KEYS = {
    "eos.primary.scale.pressure": "the library's pressure scale stays 1e6 (another scaling, another Newton path)",
    "eos.primary.scale.temperature": "the library's temperature scale stays 100 (another scaling, another Newton path)",
    "eos.primary.scale.partial_pressure": "the gas partial pressure keeps its adaptive scaling",
    "initial.minc": "whether the initial conditions hold the MINC cells is read off their size",
    "mesh.minc.additionalProperties": "the schema lists it; the reference reads no such key",
    "mesh.minc.rock.cells": "MINC zones are given by rock types or zones",
    "mesh.zones.*.*": "zones made of other zones", "mesh.zones.*.+": "zones made of other zones",
    "mesh.zones.*.-": "zones made of other zones", "mesh.zones.*.r": "zones by radius",
    "output.checkpoint.step": "output checkpoints by step size",
    "output.jacobian": "no Jacobian file is written", "output.jacobian.filename": "no Jacobian file is written",
    "source.cells": "sources given by cell lists", "source.zones": "sources given by zones",
    "source.rate.time": "source rate given as an object", "source.enthalpy.time": "source enthalpy given as an object",
    "source.injectivity.pressure.enthalpy": "injectivity reference pressure against enthalpy",
    "source.recharge.pressure.enthalpy": "recharge reference pressure against enthalpy",
    "source.tracer.*": "tracer injection rates given by tracer name",
    "time.step.solver.nonlinear.jacobian": "finite-difference increments of the Jacobian",
    "time.step.solver.nonlinear.jacobian.differencing": "finite-difference increments of the Jacobian",
    "time.step.solver.nonlinear.jacobian.differencing.increment": "finite-difference increments of the Jacobian",
    "time.step.solver.nonlinear.jacobian.differencing.tolerance": "finite-difference increments of the Jacobian",
    "time.step.solver.nonlinear.tolerance.update": "convergence on the size of the Newton update",
    "time.step.solver.nonlinear.tolerance.update.absolute": "convergence on the size of the Newton update",
    "time.step.solver.nonlinear.tolerance.update.relative": "convergence on the size of the Newton update",
    "time.step.stop": "stopping on the step size", "time.step.stop.size": "stopping on the step size",
    "time.step.stop.size.maximum": "stopping on the step size", "time.step.stop.size.minimum": "stopping on the step size",
}
KEY_TABLE = dict({k: "handled" for k in HANDLED_KEYS.split()}, **{k: "no effect" for k in NO_EFFECT_KEYS.split()})
KEY_TABLE.update({k: "refused" for k in REFUSED_KEYS})


def schema_path(path):
    """a key path as the schema's walk writes it ("source[].rate", "boundaries[].faces[].cells") in KEY_TABLE's normal form"""
    return path.replace("[]", "")


def check_input_keys(inp):
    """walks an input and raises NotImplementedError, naming the full path, for the first key that is refused or that
    KEY_TABLE does not hold (no key of the reference's schema: nothing would read it).  A key whose value is null counts
    as absent, as everywhere here.  Pure: the input alone, so before any library and the same on every rank."""
    def walk(node, shown, norm):
        if isinstance(node, dict):
            for k, v in node.items():
                if v is None:
                    continue
                p = norm + "." + k if norm else k
                if p not in KEY_TABLE and norm + ".*" in KEY_TABLE:
                    p = norm + ".*"
                s = shown + "." + k if shown else k
                kind = KEY_TABLE.get(p)
                if kind is None:
                    raise NotImplementedError("input key %s (%s) is no key of the reference's input schema: nothing reads it" % (s, p))
                if kind == "refused":
                    raise NotImplementedError("input key %s (%s) is not supported: %s" % (s, p, REFUSED_KEYS[p]))
                walk(v, s, p)
        elif isinstance(node, (list, tuple)):
            for i, v in enumerate(node):
                walk(v, "%s[%d]" % (shown, i), norm)
    walk(inp, "", "")


def component_index(name, eos, key="component"):
    """"component" / "production_component" of a source as the reference's get_component takes it (src/source_setup.F90:2030-
    2049, eos_component_index, src/eos.F90:261-281): an integer, or a name -- "water", the EOS's second and third mass
    components by name ("gas" for the non-condensible gas whichever it is), "energy" for the last, heat, equation"""
    if isinstance(name, (int, np.integer)) and not isinstance(name, bool):
        return int(name)
    names = {"w": ["water"], "we": ["water"], "wce": ["water", "co2"], "wae": ["water", "air"], "wse": ["water", "salt"],
             "wsce": ["water", "salt", "co2"], "wsae": ["water", "salt", "air"]}[eos]
    low = str(name).strip().lower()
    if low == "energy" and eos != "w":
        return len(names) + 1
    if low == "gas" and names[-1] in ("co2", "air"):
        return len(names)
    if low in names:
        return names.index(low) + 1
    raise ValueError("source %s %r: eos %s has the components %s%s" % (key, name, eos, names, "" if eos == "w" else " and energy"))


def production_components(inp, eos):
    """"source[].production_component" of every source as integers (0: none named, production follows "component" as
    before), and what the key does not combine with here refused by name, from the input alone.  In the reference a
    production component only chooses where the produced rate goes (source.F90:403-453): deliverability, recharge, a limiter on
    the total flow, direction and factor set the RATE and combine with it as they are.  A separator, a limiter on separated
    water or steam and a source network separate or pass on the flow by its enthalpy, which a heat-only source does not
    form: not built, refused."""
    sources = inp.get("source", []) or []
    net = inp.get("network") or {}
    members = set()
    for g in net.get("group") or []:
        members.update(g.get("in") or [])
    for r in net.get("reinject") or []:
        members.add(r.get("in"))
        for key in ("water", "steam"):
            members.update(o.get("out") for o in r.get(key) or [])
        over = r.get("overflow")
        members.add(over.get("out") if isinstance(over, dict) else over)
    np_ = {"w": 1, "we": 2, "wce": 3, "wse": 3, "wae": 3, "wsce": 4, "wsae": 4}[eos]
    out = []
    for i, s in enumerate(sources):
        if s.get("production_component") is None:
            out.append(0)
            continue
        c = component_index(s["production_component"], eos, "production_component")
        if c > np_:
            raise ValueError("source[%d].production_component %r: eos %s has %d equations" % (i, s["production_component"], eos, np_))
        lim = s.get("limiter") or {}
        met = ("source[%d].separator" % i if s.get("separator") not in (None, False)
               else "source[%d].limiter on separated %s" % (i, lim.get("type") if lim.get("type") in ("water", "steam") else
                                                             "water" if "water" in lim else "steam")
               if (lim.get("type") in ("water", "steam") or "water" in lim or "steam" in lim or "separator_pressure" in lim)
               else "membership of the source network (network.group / network.reinject)" if s.get("name") is not None and s["name"] in members
               else None)
        if c > 0 and met:
            raise NotImplementedError("source[%d].production_component together with %s" % (i, met))
        out.append(max(c, 0))
    return out


# the reference's defaults of the auxiliary (tracer) solver where its "auxiliary" object leaves a key out
# (default_auxiliary_ksp_type_str / default_auxiliary_pc_type_str, src/timestepper.F90:2021-2022; PETSc's rtol)
AUXILIARY_DEFAULTS = {"ksp_type": "gmres", "ksp_rtol": 1.0e-5}
AUXILIARY_DEFAULT_PC = "bjacobi"


def linear_solver_options(obj, default_pc, sub_lu="host", defaults=None):
    """One linear-solver object of the input ("time.step.solver.linear" or "time.step.solver.auxiliary": the same keys,
    src/timestepper.F90:1645-1836, 2057-2065) -> the library's options.  Pure: no library, no device.

    Keys read: type, tolerance.relative, maximum.iterations, options.gmres.restart, preconditioner.type,
    preconditioner.sub.preconditioner.{type, factor.levels}.  default_pc: the preconditioner of an object that names none;
    sub_lu: the mapping of sub-preconditioner lu under bjacobi / asm (module docstring); defaults: options an object that
    leaves them out gets (None: only what the object names is set).

    Returns dict(opts: ksp_type, ksp_rtol, ksp_max_its, gmres_restart (where named, or in defaults), pc_type, ilu_levels;
    sub_device: the library's sub-preconditioner lu is to be set; pc: the preconditioner's name as taken; named: whether the
    object named it; note: () or one sentence on how sub lu was mapped).  Unknown types raise NotImplementedError."""
    lin = obj or {}
    opts = dict(defaults or {})
    if lin.get("type") in ("bcgs", "gmres", "bcgsl", "lgmres"):
        opts["ksp_type"] = lin["type"]
    elif lin.get("type") is not None:
        raise NotImplementedError("linear solver type %r" % lin["type"])
    if _get(lin, "tolerance.relative") is not None:
        opts["ksp_rtol"] = lin["tolerance"]["relative"]
    if _get(lin, "maximum.iterations") is not None:
        opts["ksp_max_its"] = lin["maximum"]["iterations"]
    if _get(lin, "options.gmres.restart") is not None:
        opts["gmres_restart"] = lin["options"]["gmres"]["restart"]
    # preconditioner (src/timestepper.F90:1745-1757); "ilu" of a serial run is the one-block case of bjacobi / asm.
    # Sub-preconditioner ilu with "factor.levels" k (ILU(k), :1716-1718, 1827) or lu.
    pct_in = _get(lin, "preconditioner.type")
    pct = (pct_in or default_pc).lower()
    if pct not in ("asm", "bjacobi", "ilu", "lu", "none"):
        raise NotImplementedError("preconditioner type %r" % pct)
    opts["pc_type"] = {"ilu": "bjacobi"}.get(pct, pct)
    sub = _get(lin, "preconditioner.sub.preconditioner", {}) or {}
    subt = (sub.get("type") or "ilu").lower()
    sub_device, note = False, ()
    if subt == "lu" and pct in ("bjacobi", "asm") and sub_lu == "device":
        # exact solves of the (overlapped) blocks on the device: the outer preconditioner stays what the input names
        sub_device = True
        note = ("sub lu: exact block solves on the device (wai_set_sub_pc)",)
    elif subt == "lu" and pct in ("bjacobi", "asm"):
        opts["pc_type"] = "lu"       # exact block solves (block Jacobi; no overlap)
        note = ("sub lu: dense block inverses from the host, block Jacobi%s" % (" (the overlap is dropped)" if pct == "asm" else ""),)
    elif subt != "ilu":
        raise NotImplementedError("sub-preconditioner %r" % (sub,))
    else:
        levels = int(_get(sub, "factor.levels") or 0)
        if levels and opts["pc_type"] not in ("asm", "bjacobi"):
            raise NotImplementedError("factor.levels needs a block Jacobi or ASM preconditioner")
        opts["ilu_levels"] = levels
    return dict(opts=opts, sub_device=sub_device, pc=pct, named=pct_in is not None, note=note)


def pc_coarse_refusal(lso, has_network, world, has_tracers, multicolour):
    """what the coarse level (pc_coarse="additive" | "deflated", wai_set_pc_coarse) does not combine with, from the input's
    solver object and the arguments alone, so every rank decides alike: None, or the refusal's text"""
    met = None
    if world > 1:
        met = "more than one rank"
    elif has_network:
        met = "a source network (its couplings are part of the operator)"
    elif lso["opts"].get("pc_type") in ("none", "lu"):
        met = "preconditioner %r" % lso["opts"]["pc_type"]
    elif multicolour:
        met = "pc_ordering 'multicolour'"
    elif has_tracers:
        met = "tracers (the auxiliary systems)"
    return None if met is None else "pc_coarse serves the flow solver under bjacobi or asm on one rank; the input and arguments give " + met


def coarse_aggregates_of(lm, n_aggregates):
    """aggregates for the coarse level from the library's coordinate bisection (wai_cell_order with the cap
    ceil(n / n_aggregates)): the aggregate of every owned cell, its leaves numbered in order.  The cell order handed to the
    library is not changed"""
    from . import lib as wl
    n = lm.n_owned
    if n_aggregates < 1:
        raise ValueError("coarse_aggregates: at least 1")
    faces = np.asarray(lm.face_cells).reshape(-1, 2)
    interior = faces[(faces[:, 0] < n) & (faces[:, 1] < n)]
    perm, leaves = wl.cell_order(interior, np.asarray(lm.cell_geom)[:n, :3], -(-n // int(n_aggregates)))
    agg = np.empty(n, dtype=np.int32)
    agg[perm] = np.repeat(np.arange(len(leaves) - 1), np.diff(leaves))
    return agg


def pc_ordering_refusal(lso, has_network):
    """what the multicolour ordering (pc_ordering="multicolour", wai_set_pc_ordering) does not combine with, from
    linear_solver_options' result for the flow solver and whether the input has a source network: a sentence that names the
    setting and what it met, or None.  Pure -- the input and the arguments alone, so every rank decides alike.  Block Jacobi
    with ILU(0) is served; under "none" and the dense "lu" the setting is ignored, as in the library."""
    o = lso["opts"]
    met = None
    if o.get("pc_type") == "asm":
        met = "preconditioner asm"
    elif lso["sub_device"]:
        met = "sub-preconditioner lu on the device (sub_lu='device')"
    elif o.get("ilu_levels"):
        met = "sub-preconditioner ilu with factor.levels %d (ILU(k))" % o["ilu_levels"]
    elif has_network and o.get("pc_type") == "bjacobi":
        met = "a source network (its Jacobian blocks go into the factor's pattern)"
    return None if met is None else "pc_ordering 'multicolour' serves bjacobi with ILU(0) alone; the input and arguments give " + met


def covers_coupled(lso):
    """does the coupled tracer solve cover the preconditioner of linear_solver_options' result: block Jacobi ILU(0) or none"""
    o = lso["opts"]
    return o.get("pc_type", "bjacobi") in ("bjacobi", "none") and not o.get("ilu_levels") and not lso["sub_device"]


def relperm_spec(rp):
    """rock.relative_permeability -> (type, parameters) of the library's EOS descriptor"""
    if rp is None:
        return "linear", [0.0, 1.0, 0.0, 1.0]
    t = rp.get("type", "linear").lower()
    if t == "linear":
        return "linear", list(rp.get("liquid", [0.0, 1.0])) + list(rp.get("vapour", [0.0, 1.0]))
    if t in ("fully mobile", "fully_mobile"):
        return "fully_mobile", []
    if t in ("corey", "grant"):
        return t, [rp.get("slr", 0.3), rp.get("ssr", 0.05 if t == "corey" else 0.6)]
    if t == "pickens":
        return "pickens", [rp.get("power", 1.0)]
    if t in ("van genuchten", "van_genuchten"):
        return "van_genuchten", [rp.get("lambda", 0.45), rp.get("slr", 1.0e-3), rp.get("sls", 1.0),
                                 1.0 if rp.get("sum_unity", True) else 0.0, rp.get("ssr", 0.6)]
    if t == "table":   # src/relative_permeability.F90:500-543
        spec = {"interpolation": rp.get("interpolation", "linear")}
        for k in ("liquid", "vapour"):
            if rp.get(k) is not None:
                spec[k] = [list(map(float, row)) for row in rp[k]]
        return "table", spec
    raise NotImplementedError("relative permeability type %r" % t)


def capillary_spec(cp):
    if cp is None:
        return "zero", []
    t = cp.get("type", "zero").lower()
    if t == "zero":
        return "zero", []
    if t == "linear":
        s = cp.get("saturation_limits", [0.0, 1.0])
        if cp.get("pressure", 0.125e5) == 0:
            return "zero", []
        return "linear", [s[0], s[1], cp.get("pressure", 0.125e5)]
    if t in ("van genuchten", "van_genuchten"):
        pmax = cp.get("Pmax")
        return "van_genuchten", [cp.get("P0", 0.125e5), cp.get("lambda", 0.45), cp.get("slr", 1.0e-3),
                                 cp.get("sls", 1.0), pmax if pmax is not None else 0.0, 1.0 if pmax is not None else 0.0]
    if t == "table":   # src/capillary_pressure.F90:311-345
        spec = {"interpolation": cp.get("interpolation", "linear")}
        if cp.get("pressure") is not None:
            spec["pressure"] = [list(map(float, row)) for row in cp["pressure"]]
        return "table", spec
    raise NotImplementedError("capillary pressure type %r" % t)


def _is_table(v):
    """a rank-2 array: rows of [time, value(s)] (rock_setup.F90:300-326: permeability of rank 2, porosity any array)"""
    return isinstance(v, (list, tuple)) and len(v) > 0 and isinstance(v[0], (list, tuple))


def rock_record(rt, dim):
    k = rt.get("permeability", 1.0e-13)
    if _is_table(k):       # permeability against time: a rock control sets it before every try; start from the first row
        k = list(k[0][1:])
    por = rt.get("porosity", 0.1)
    if isinstance(por, (list, tuple)):
        rt = dict(rt, porosity=(por[0][1] if _is_table(por) else por[0]))
    k = [k] * 3 if np.isscalar(k) else list(k) + [k[-1]] * (3 - len(k))
    return np.array([k[0], k[1], k[2], rt.get("wet_conductivity", 2.5), rt.get("dry_conductivity", rt.get("wet_conductivity", 2.5)),
                     rt.get("porosity", 0.1), rt.get("density", 2200.0), rt.get("specific_heat", 1000.0)])


def zone_cells(zone, centroids):
    """cells of a "mesh.zones" entry: box ranges on x / y / z (a box without ranges is everything)"""
    if zone is None:
        return np.arange(len(centroids))
    if isinstance(zone, dict):
        if "cells" in zone:
            return np.asarray(zone["cells"], dtype=int)
        sel = np.ones(len(centroids), dtype=bool)
        for ax, name in enumerate("xyz"):
            if name in zone and zone[name] is not None:
                lo, hi = zone[name]
                sel &= (centroids[:, ax] >= lo) & (centroids[:, ax] <= hi)
        unknown = set(zone) - {"x", "y", "z", "type", "cells"}
        if unknown:
            raise NotImplementedError("mesh zone keys %s" % sorted(unknown))
        return np.nonzero(sel)[0]
    raise NotImplementedError("mesh zone %r" % (zone,))


def network_spec(inp, interval, separator_enthalpies=None):
    """"network": {"group": [...], "reinject": [...]} of an input file (setup_source_network_groups /
    _reinjectors, src/source_setup.F90) as the description waiwera_amd.lib.network_arrays flattens for
    wai_set_source_network.  Rates, proportions and enthalpies given as time tables are averaged over
    `interval` (table_object_control_update, src/control.F90:263-284).  Returns (spec or None, names of
    the groups / reinjectors in spec order, whether anything is a time table)."""
    net = inp.get("network") or {}
    groups, reinj = list(net.get("group") or []), list(net.get("reinject") or [])
    names = {"group": [g.get("name", "") for g in groups], "reinject": [r.get("name", "") for r in reinj]}
    if not groups and not reinj:
        return None, names, False
    sources = inp.get("source", []) or []
    sidx = {s["name"]: i for i, s in enumerate(sources) if "name" in s}
    gnames = [g.get("name", "") for g in groups]
    order, done = [], set()
    while len(order) < len(groups):      # groups in dependency order
        progress = False
        for gi, g in enumerate(groups):
            if gi in done:
                continue
            if all(n in sidx or (n in gnames and gnames.index(n) in done) for n in g.get("in", [])):
                order.append(gi); done.add(gi); progress = True
        if not progress:
            raise ValueError("network groups refer to unknown nodes or to each other in a cycle")
    groups = [groups[gi] for gi in order]
    gidx = {g.get("name", ""): k for k, g in enumerate(groups)}
    ridx = {r.get("name", ""): k for k, r in enumerate(reinj)}
    names["group"] = [g.get("name", "") for g in groups]
    timed = [False]

    def ref(name, allowed):
        for kind, table in ((1, sidx), (2, gidx), (3, ridx)):
            if kind in allowed and name in table:
                return kind, table[name]
        raise ValueError("network node %r not found" % (name,))

    def value(v, o, default):
        if v is None:
            return default
        if isinstance(v, dict):
            v = v.get("time")
        if isinstance(v, (list, tuple)):
            timed[0] = True
            return float(Table(v, o.get("interpolation", "linear"), o.get("averaging", "integrate")).average(interval)[0])
        return float(v)

    def separator(sp):
        if not sp:
            return None
        if separator_enthalpies is None:
            raise NotImplementedError("separator on a network group needs the thermodynamics (separator_enthalpies)")
        ps = sp.get("pressure", 0.55e6) if isinstance(sp, dict) else 0.55e6
        ps = list(ps) if isinstance(ps, (list, tuple)) else [ps]
        if len(ps) > 4:
            raise NotImplementedError("separators with more than 4 stages")
        return [separator_enthalpies(float(q)) for q in ps]
    FLOW = {"total": 0, "water": 1, "steam": 2}
    # rate_specified: a "rate" in the input (source_setup.F90:2087-2118, get_initial_rate) -- or a deliverability
    # (:2911) or recharge / injectivity (:3081) control, whose set-up sets source%rate_specified = PETSC_TRUE; the
    # control's rate then becomes the specified rate with every source%set_rate (source.F90:276-288), so a
    # reinjector output into such a well is capped by what the control gives (source.F90:292-303)
    spec = dict(rate_specified=[int("rate" in s or any(k in s for k in ("deliverability", "recharge", "injectivity")))
                                for s in sources],
                enthalpy_specified=[int("enthalpy" in s) for s in sources], groups=[], reinjectors=[])
    for g in groups:
        lim = g.get("limiter") or {}
        if "type" in lim:
            lim = {lim["type"]: lim.get("limit")}
        limits = [(FLOW[k], value(lim[k], lim, 0.0)) for k in ("total", "water", "steam") if lim.get(k) is not None]
        spec["groups"].append(dict(inputs=[ref(n, (1, 2)) for n in g.get("in", [])],
                                   scaling={"uniform": 0, "progressive": 1}[g.get("scaling", "uniform")], limits=limits,
                                   separator=separator(g.get("separator"))))
    for r in reinj:
        outs = []
        for flow, key in ((1, "water"), (2, "steam")):
            for o in r.get(key) or []:
                has_rate = o.get("rate") is not None
                outs.append(dict(flow=flow, out=ref(o["out"], (1, 3)) if o.get("out") else (0, -1),
                                 rate=value(o.get("rate"), o, -1.0),
                                 proportion=value(o.get("proportion"), o, -1.0) if not has_rate else -1.0,
                                 enthalpy=value(o.get("enthalpy"), o, -1.0)))
        over = r.get("overflow")
        if isinstance(over, dict):
            over = over.get("out")
        spec["reinjectors"].append(dict(input=ref(r["in"], (1, 2)) if r.get("in") else (0, -1), outputs=outs,
                                        overflow=ref(over, (1, 3)) if over else (0, -1)))
    return spec, names, timed[0]


def face_output(face_cells, n_prim, n_bc, bc_spec, area):
    """(face_cell_1, face_cell_2, face_geometry_area) of an output file from a mesh's faces: a face's second cell that is a
    Dirichlet boundary cell (numbered from n_prim on) reads -1 - the index of the boundary specification it belongs to"""
    fc = np.asarray(face_cells).reshape(-1, 2)
    c2 = fc[:, 1].astype(np.int64)
    bnd = c2 >= n_prim
    spec = np.asarray(bc_spec)
    c2 = np.where(bnd, -1 - spec[np.clip(c2 - n_prim, 0, max(n_bc - 1, 0))], c2) if spec.size else c2
    return fc[:, 0].copy(), c2, np.asarray(area).copy()


def output_datasets(outs, n_cells, minc_level=None, minc_parent=None):
    """The datasets of an output file in the reference's layout from a list of snapshots (dicts as Simulation.fields()
    returns them, each of the same n_cells cells): /time, /cell_index, /cell_fields/*, /source_fields/* (sources and network
    nodes), /face_fields/* with /face_cell_1 and /face_cell_2, and -- given the MINC level and parent of every cell in the
    output's cell order (flow_simulation_output_minc_data, src/flow_simulation.F90:2625-2691: level 0 a fracture or
    single-porosity cell, parent the natural index of the original cell) -- /minc/level and /minc/parent.  Pure: no
    library, no file; one rank and the root of N ranks build the file's contents here."""
    data = {"/time": np.array([[o["time"]] for o in outs]), "/cell_index": np.arange(n_cells, dtype=np.int32)[:, None]}
    if minc_level is not None:
        data["/minc/level"] = np.asarray(minc_level).astype(np.int32)[:, None]
        data["/minc/parent"] = np.asarray(minc_parent).astype(np.int32)[:, None]
    for k in outs[0]:
        if k == "time":
            continue
        if k.startswith("source_") or k.startswith("network_"):
            data["/source_fields/" + k] = np.stack([o[k] for o in outs])
        elif k.startswith("flux_"):
            data["/face_fields/" + k] = np.stack([o[k] for o in outs])
        elif k.startswith("face_geometry"):
            data["/face_fields/" + k] = outs[0][k]
        elif k.startswith("face_cell_"):
            data["/" + k] = np.asarray(outs[0][k], dtype=np.int32)[:, None]
        elif k.startswith("cell_geometry"):
            data["/cell_fields/" + k] = outs[0][k]
        else:
            data["/cell_fields/" + k] = np.stack([o[k] for o in outs])
    return data


CellOrderChoice = collections.namedtuple("CellOrderChoice", "order n_sub largest_subdomain cut_before cut_after")
CellOrderChoice.__doc__ = """Simulation.cell_order_choice: the order taken ("input" | "compact"), the preconditioner subdomains it gives and
the largest one's cells, and the share of interior faces cut by the input-order chunks (before) and by the subdomains taken (after)"""


def _cut_share(interior, sub_ptr):
    """share of the interior faces (cell pairs) whose cells lie in different subdomains"""
    interior = np.asarray(interior).reshape(-1, 2)
    if not len(interior):
        return 0.0
    owner = np.repeat(np.arange(len(sub_ptr) - 1), np.diff(np.asarray(sub_ptr, dtype=np.int64)))
    return float(np.mean(owner[interior[:, 0]] != owner[interior[:, 1]]))


def _face_places(input_faces, faces, perm, n):
    """for the faces of the mesh numbered by perm[new] = old: (each one's place in the input-order mesh's face list, whether
    it is oriented the other way round there).  Cells from n on are boundary cells, the same in both meshes"""
    old = np.asarray(faces, dtype=np.int64).copy()
    own = old < n
    old[own] = np.asarray(perm, dtype=np.int64)[old[own]]
    ref = np.asarray(input_faces, dtype=np.int64)
    big = max(int(ref.max(initial=0)), int(old.max(initial=0))) + 1
    key = lambda f: f.min(axis=1) * big + f.max(axis=1)     # noqa: E731
    a, b = np.argsort(key(ref), kind="stable"), np.argsort(key(old), kind="stable")
    if len(ref) != len(old) or not np.array_equal(key(ref)[a], key(old)[b]):
        raise RuntimeError("the mesh in compact cell order has other faces than the mesh in input order")
    place = np.empty(len(old), dtype=np.int64)
    place[b] = a
    return place, old[:, 0] != ref[place, 0]


def renumber_input(inp, perm, inv):
    """a copy of the input with every cell number it carries put through inv (inv[old] = new) and every per-cell array
    listed in the new order (perm[new] = old): boundaries[].faces.cells, source[].cell, rock.types[].cells, mesh.faces[].cells,
    zones given as cell lists, per-cell initial.primary / region / tracer.  Pure."""
    import copy
    out = copy.deepcopy(inp)
    n = len(perm)
    renum = lambda cells: [int(inv[c]) for c in cells]      # noqa: E731
    for b in out.get("boundaries") or []:
        faces = b.get("faces")
        for f in (faces if isinstance(faces, list) else [faces]):
            if isinstance(f, dict) and f.get("cells") is not None:
                f["cells"] = renum(f["cells"])
    for s_ in out.get("source") or []:
        if s_.get("cell") is not None:
            s_["cell"] = int(inv[s_["cell"]])
    for rt in (out.get("rock") or {}).get("types") or []:
        if rt.get("cells") is not None:
            rt["cells"] = renum(rt["cells"])
    mesh = out.get("mesh")
    for z in ((mesh.get("zones") or {}) if isinstance(mesh, dict) else {}).values():
        if isinstance(z, dict) and z.get("cells") is not None:
            z["cells"] = renum(z["cells"])
    for f in ((mesh.get("faces") or []) if isinstance(mesh, dict) else []):
        if f.get("cells") is not None:
            f["cells"] = renum(f["cells"])
    init = out.get("initial") or {}
    for key, rank in (("primary", 2), ("region", 1), ("tracer", 2)):
        v = init.get(key)
        if isinstance(v, (list, tuple)) and np.ndim(v) == rank and len(v) == n:
            init[key] = [v[p] for p in perm]
    return out


class Simulation:
    """One Waiwera input file -> mesh, flow simulation object and time stepper."""

    def __init__(self, inp, base_dir=".", ode_factory=None, device=0, mesh_builder=None, mesh_file=None,
                 output_dir=None, rank=0, world=1, comm_id=None, owner=None, default_pc="asm", tracer_solve="per_tracer",
                 sub_lu="host", default_aux_pc=None, subdomains="chunks", pc_ordering="natural", network_pass="host",
                 cell_order="input", subdomain_rows=None, coupling_build="columns", network_walk="lane", pc_coarse=None,
                 coarse_aggregates=64):
        """rank / world / comm_id (wai_comm_unique_id of rank 0, handed round by the host): one process per rank, each
        reads the whole input, keeps its own cells with one ghost layer (waiwera_amd.partition.partition_mesh; owner: rank of
        every cell, default contiguous blocks of the input's numbering; a MINC mesh: per input cell, or per cell in the
        output's order with every family on one rank, waiwera_amd.partition.family_owner) and runs the same step sequence --
        what DMPlexDistribute (src/mesh.F90:143-171) does for the reference.  What N ranks cover: the module docstring
        (fields() returns the rank's cells, self.owned_gid their index in the one-rank output's numbering)."""
        self.rank, self.world = int(rank), int(world)
        # every key of the input is honoured, without effect or refused by name (KEY_TABLE): before anything is read, built
        # or handed to the library, and from the input alone, so on every rank alike
        check_input_keys(inp)
        # tracer_solve: "per_tracer" (one scalar solve per tracer) or "coupled" (all tracers in one Krylov solve, as the
        # reference; needs the bjacobi or no preconditioner).  Not a key of the input file: the reference has none
        if tracer_solve not in ("per_tracer", "coupled"):
            raise ValueError("tracer_solve 'per_tracer' or 'coupled'")
        self.tracer_solve = tracer_solve
        if default_pc not in ("asm", "bjacobi"):
            raise ValueError("default_pc 'asm' (the reference's default) or 'bjacobi' (the library's fused path)")
        self.default_pc, self.pc_choice = default_pc, None
        # default_aux_pc: the tracer solver's preconditioner for an input without "time.step.solver.auxiliary" -- None: the
        # flow solver's (the library's default, as before), "bjacobi": the reference's auxiliary default, or "asm".  An input
        # WITH the object gets what it names, and the reference's auxiliary defaults for what it leaves out
        if default_aux_pc not in (None, "asm", "bjacobi"):
            raise ValueError("default_aux_pc None (the tracer solves follow the flow solver), 'bjacobi' (the reference's default) or 'asm'")
        self.default_aux_pc, self.aux_pc_choice = default_aux_pc, None
        # sub_lu: how sub-preconditioner "lu" under bjacobi / asm is mapped (module docstring): "host" dense block inverses
        # without overlap (the default: no earlier result moves), "device" the library's sub-preconditioner lu
        if sub_lu not in ("host", "device"):
            raise ValueError("sub_lu 'host' (dense block inverses, no overlap) or 'device' (exact LU of the blocks on the device)")
        self.sub_lu = sub_lu
        # pc_ordering: elimination order of the flow solver's block-Jacobi ILU(0) -- "natural" (the default: the reference's
        # ILU(0)) or "multicolour" (wai_set_pc_ordering: two sweep levels per brick on hexahedral and MINC meshes; another
        # preconditioner, so other Krylov counts).  Not a key of the input file: the reference has none.  What it does not
        # combine with is refused when the solver options are read (pc_ordering_refusal); pc_choice records it
        if pc_ordering not in ("natural", "multicolour"):
            raise ValueError("pc_ordering 'natural' (the default) or 'multicolour'")
        self.pc_ordering = pc_ordering
        # pc_coarse: a coarse level for the flow solver's preconditioner -- None (the default: one level, as before),
        # "additive" or "deflated" (wai_set_pc_coarse: piecewise constant over coarse_aggregates aggregates from the library's
        # coordinate bisection, Galerkin, inverted densely on the device; another preconditioner, so other Krylov counts).
        # Not a key of the input file: the reference has none.  What it does not combine with is refused when the solver
        # options are read (pc_coarse_refusal); pc_choice records the mode and the number of aggregates
        if pc_coarse not in (None, "additive", "deflated"):
            raise ValueError("pc_coarse None (the default), 'additive' or 'deflated'")
        self.pc_coarse, self.coarse_aggregates = pc_coarse, int(coarse_aggregates)
        # network_pass: where the source network's pass runs -- "host" (the default, as before) or "device"
        # (wai_set_network_pass: one launch in LDS, the coupling build without waits inside; the same bits).  Not a key of the
        # input file.  network_pass_choice records (requested, in force) once the network is set: "host" stays in force on
        # several ranks and for a network too large for a workgroup's LDS
        if network_pass not in ("host", "device"):
            raise ValueError("network_pass 'host' (the default) or 'device'")
        self.network_pass, self.network_pass_choice = network_pass, (network_pass, "host")
        # coupling_build: how the Jacobian's blocks through the source network are built -- "columns" (the default, as
        # before: one column at a time) or "batched" (wai_set_coupling_build: all columns at once on private scratch; the
        # same bits).  Not a key of the input file.  coupling_build_choice records (requested, in force) once the network is
        # set: "batched" is in force where network_pass "device" is
        if coupling_build not in ("columns", "batched"):
            raise ValueError("coupling_build 'columns' (the default) or 'batched'")
        self.coupling_build, self.coupling_build_choice = coupling_build, (coupling_build, "columns")
        # network_walk: how the device pass walks groups and reinjectors -- "lane" (the default, as before: one lane) or "wave"
        # (wai_set_network_walk: the wave's lanes gather, one chains; networks of up to 160 KiB of LDS; the same bits).  Not a
        # key of the input file.  network_walk_choice records (requested, in force) once the network is set: "wave" is in
        # force where network_pass "device" is and the wave schedule accepts the network
        if network_walk not in ("lane", "wave"):
            raise ValueError("network_walk 'lane' (the default) or 'wave'")
        self.network_walk, self.network_walk_choice = network_walk, (network_walk, "lane")
        # subdomains: the preconditioner's blocks on a rank -- "chunks" (the default, as before): the chunks of consecutive cells
        # the mesh builders make (mesh.sub_ptr), each on the fused one-workgroup kernels; "rank": ONE block per rank, the
        # reference's own layout (its bjacobi / asm subdomains are the ranks), with the same chunks handed to the library as
        # tiles (set_pc_tiles), so that the block's sweeps take a launch per level of chunks instead of one per level of rows
        # where that is fewer.  subdomain_choice records what was taken
        if subdomains not in ("chunks", "rank"):
            raise ValueError("subdomains 'chunks' (the mesh's chunks, the default) or 'rank' (one block per rank, the reference's layout)")
        self.subdomains, self.subdomain_choice = subdomains, None
        # cell_order: the numbering the library gets -- "input" (the default, as before): the mesh file's, with chunks of
        # consecutive cells as the preconditioner's subdomains; "compact" (wai_cell_order): compact 3-D subdomains of at most
        # subdomain_rows cells, numbered inside like a brick.  Everything the input says by cell number goes in through the
        # inverse permutation and every result comes back in the input's numbering; cell_order_choice records the order taken,
        # the subdomains and the share of interior faces they cut.  subdomain_rows: the cap under either order (None: 512, or
        # 512 // (1 + MINC levels)).  Not keys of the input file: the reference partitions through DMPlex
        if cell_order not in ("input", "compact"):
            raise ValueError("cell_order 'input' (the mesh file's numbering, the default) or 'compact' (compact subdomains, wai_cell_order)")
        if subdomain_rows is not None and (isinstance(subdomain_rows, bool) or not isinstance(subdomain_rows, (int, np.integer))
                                           or not 1 <= subdomain_rows <= 1024):
            raise ValueError("subdomain_rows None (512 rows, MINC cells included) or an integer from 1 to 1024")
        self.cell_order, self.subdomain_rows, self.cell_order_choice = cell_order, subdomain_rows, None
        self._perm = self._inv = self._input_faces = None
        # output files go to output_dir (default: $WAIWERA_OUTPUT_DIR, else beside the input file)
        self.output_dir = output_dir or os.environ.get("WAIWERA_OUTPUT_DIR") or base_dir
        self.output_error = None
        self.inp = inp
        self.base_dir = base_dir
        mesh = inp.get("mesh")
        if isinstance(mesh, str):
            mesh = {"filename": mesh}
        if self.cell_order == "compact":
            # from the arguments and the input alone, before anything is built or exchanged: each of these numbers the cells
            # itself (partition_mesh, the mesh_builder, add_minc_zones' waiwera_order) and needs its own composition with perm
            met = ("world = %d ranks" % self.world if self.world > 1 else "a mesh_builder" if mesh_builder is not None
                   else "MINC zones (mesh.minc)" if (mesh or {}).get("minc") else None)
            if met:
                raise ValueError("cell_order 'compact' serves one rank, a mesh file and no MINC zones; the input and arguments give " + met)
        if mesh_builder is None:
            # gmsh 2.2 ASCII, or (mesh_file: the input names an ExodusII file, which cannot be read
            # here) the MULgraph geometry file the reference's benchmarks keep beside it
            mpath = mesh_file or os.path.join(base_dir, mesh["filename"])
            if mpath.endswith(".dat"):
                from . import mulgrid
                nodes, cells, dim = mulgrid.read_geometry(mpath)
            else:
                nodes, cells, dim = gmsh.read_msh(mpath)
            n = len(cells)
        else:
            # mesh_builder(boundaries, sources) -> LocalMesh for meshes that are not gmsh files (the
            # ExodusII meshes of some reference benchmarks are rebuilt from their description);
            # mesh_builder.dim, mesh_builder.n_cells describe it
            dim, n = mesh_builder.dim, mesh_builder.n_cells
        self.dim = dim
        # gravity (flow_simulation.F90:800-846)
        gin = inp.get("gravity")
        grav = np.zeros(3)
        if isinstance(gin, (list, tuple)):
            grav[: len(gin)] = gin
        else:
            grav[dim - 1] = -(gin if gin is not None else (0.0 if dim == 2 else 9.8))
        # EOS and thermodynamics
        eos = inp.get("eos", "we")
        self.eos = (eos.get("name", "we") if isinstance(eos, dict) else eos).lower()
        temperature = eos.get("temperature", 20.0) if isinstance(eos, dict) else 20.0
        pm = eos.get("permeability_modifier") if isinstance(eos, dict) else None
        self.permeability_modifier = None
        if pm is not None and (pm.get("type", "none").lower() != "none"):
            kind = pm["type"].lower()
            if kind == "power":
                self.permeability_modifier = ("power", [pm.get("exponent", 3.0)])
            elif kind in ("verma-pruess", "verma_pruess"):
                self.permeability_modifier = ("verma-pruess", [pm.get("exponent", 2.0), pm.get("phir", 0.1), pm.get("gamma", 0.7)])
            else:
                raise NotImplementedError("permeability modifier %r" % pm["type"])
        th = inp.get("thermodynamics", "iapws")
        self.thermo = (th.get("name", "iapws") if isinstance(th, dict) else th).lower()
        # "thermodynamics.extrapolate" (thermodynamics_setup.F90:57-89): region 1 up to 360 deg C; a bare name leaves it off
        self.thermo_extrapolate = bool(th.get("extrapolate", False)) if isinstance(th, dict) else False
        if self.eos not in ("w", "we", "wce", "wse", "wae", "wsce", "wsae") or self.thermo not in ("iapws", "ifc67"):
            raise NotImplementedError("eos %r / thermodynamics %r" % (self.eos, self.thermo))
        # geometry first without rock (centroids are needed for zones), rock filled in below
        bnds = []
        for b in inp.get("boundaries", []) or []:
            faces = b["faces"]
            for f in (faces if isinstance(faces, list) else [faces]):
                bnds.append((list(f["cells"]), list(f.get("normal", [0.0, 0.0, 1.0])), b["primary"], b.get("region", 1)))
        srcs, self._tables = [], []
        self._production_components = production_components(inp, self.eos)
        for s in inp.get("source", []) or []:
            bad = [k for k in UNSUPPORTED_SOURCE_KEYS if k in s]
            if bad:
                raise NotImplementedError("source controls %s" % bad)
            if "cell" not in s:
                raise NotImplementedError("sources given by zones or cell lists")
            # rate / enthalpy tables ([[t, value], ...]; setup_table_controls, src/source_setup.F90):
            # averaged over each step interval before the try, see _update_controls
            vals = {}
            for key, default in (("rate", 0.0), ("enthalpy", 83.9e3)):
                v = s.get(key, default)
                if isinstance(v, dict):
                    raise NotImplementedError("source %s given as an object" % key)
                if isinstance(v, (list, tuple)):
                    tab = Table(v, s.get("interpolation", "linear"), s.get("averaging", "integrate"))
                    self._tables.append((len(srcs), key, tab))
                    v = float(tab.interpolate(_get(inp, "time.start", 0.0))[0])
                vals[key] = v
            srcs.append(dict(cell=s["cell"], rate=vals["rate"], enthalpy=vals["enthalpy"],
                             component=component_index(s.get("component", 0), self.eos)))
        minc_in = (mesh or {}).get("minc")
        minc_in = [] if minc_in is None else (minc_in if isinstance(minc_in, list) else [minc_in])
        # matrix cells join their fracture cell's preconditioner subdomain (<= 1024 rows each)
        max_levels = max([len(np.atleast_1d(_get(mz, "geometry.matrix.volume", [0.9]))) for mz in minc_in] or [0])
        chunk = int(subdomain_rows) if subdomain_rows is not None else (512 // (1 + max_levels) if max_levels else 512)
        if mesh_builder is None:
            def build(cells, bnds, srcs, **kw):
                return unstructured.build_mesh(nodes, cells, dim, thickness=mesh.get("thickness", 1.0),
                                               radial=bool(mesh.get("radial", False)), gravity=grav, boundaries=bnds,
                                               sources=srcs, chunk=chunk, permeability_angle=float(mesh.get("permeability_angle") or 0.0),
                                               face_directions=[(int(f["cells"][0]), int(f["cells"][1]), f.get("permeability_direction", 1))
                                                                for f in mesh.get("faces") or [] if len(f.get("cells") or []) == 2], **kw)
            if self.cell_order == "input":
                lm = build(cells, bnds, srcs)
            else:
                # The order from the centroids and interior faces of the mesh built in input order -- with canonical_faces, so
                # that a cell's centroid is the same bits wherever the file lists it: the cells of a layer of a layered mesh
                # then share their z exactly, and another numbering of the file gives the same order.  Then the mesh build_mesh
                # makes of the same file with its elements listed in that order, the leaves as its subdomains, and the input
                # renumbered.  Of the input-order mesh the face list is kept: face results are listed and oriented by it
                from . import lib as wl
                first = build(cells, bnds, srcs, canonical_faces=True)
                interior = np.asarray(first.face_cells).reshape(-1, 2)[: first.n_faces - first.n_bc]
                perm, leaves = wl.cell_order(interior, first.cell_geom[:n, :3], chunk)
                inv = np.empty(n, dtype=np.int64)
                inv[perm] = np.arange(n)
                self._perm, self._inv = perm.astype(np.int64), inv
                inp = renumber_input(inp, perm, inv)
                mesh = inp["mesh"] if isinstance(inp.get("mesh"), dict) else mesh
                lm = build([cells[p] for p in perm], [([int(inv[c]) for c in b[0]],) + tuple(b[1:]) for b in bnds],
                           [dict(s, cell=int(inv[s["cell"]])) for s in srcs])
                lm.sub_ptr = leaves.astype(np.int32)
                faces = np.asarray(lm.face_cells).reshape(-1, 2)
                self._input_faces = np.asarray(first.face_cells).reshape(-1, 2).copy()
                self._face_place, self._face_flip = _face_places(self._input_faces, faces, perm, n)
                self.cell_order_choice = CellOrderChoice("compact", len(leaves) - 1, int(np.diff(leaves).max()),
                                                         _cut_share(interior, first.sub_ptr),
                                                         _cut_share(faces[: lm.n_faces - lm.n_bc], lm.sub_ptr))
        else:
            # (a mesh_builder makes its own face records: the two keys that change them cannot be honoured through it)
            for key in ("permeability_angle", "faces"):
                if (mesh or {}).get(key):
                    raise NotImplementedError("mesh.%s together with a mesh_builder" % key)
            lm = mesh_builder(bnds, srcs)
        cen = lm.cell_geom[:n, :3]
        rock = inp.get("rock", {}) or {}
        zones = (mesh or {}).get("zones", {}) or {}
        self._rock_controls = []     # (rock record fields, cells, Table): rock_control.F90:49-116
        for rt in rock.get("types", []) or []:
            rec = rock_record(rt, dim)
            sel = []
            if "cells" in rt and rt["cells"] is not None:
                sel.append(np.asarray(rt["cells"], dtype=int))
            if "zones" in rt and rt["zones"] is not None:
                for z in ([rt["zones"]] if isinstance(rt["zones"], str) else rt["zones"]):
                    sel.append(zone_cells(zones.get(z) if z in zones else (None if z == "all" else zones[z]), cen))
            for idx in sel:
                lm.rock[idx] = rec
            if sel and (_is_table(rt.get("permeability")) or isinstance(rt.get("porosity"), (list, tuple))):
                cells = np.unique(np.concatenate(sel)).astype(np.int32)
                interp = rt.get("interpolation", "linear")
                if _is_table(rt.get("permeability")):
                    tab = Table(rt["permeability"], interpolation=interp)
                    if tab.dim not in (1, dim):
                        raise ValueError("permeability table: 1 or %d values per row" % dim)
                    self._rock_controls.append(((0, 1, 2), cells, tab))
                if isinstance(rt.get("porosity"), (list, tuple)):
                    por = rt["porosity"] if _is_table(rt["porosity"]) else [rt["porosity"]]
                    self._rock_controls.append(((5,), cells, Table(por, interpolation=interp)))
        for k in range(lm.n_bc):
            lm.rock[n + k] = lm.rock[lm.face_cells[lm.n_faces - lm.n_bc + k, 0]]
        # MINC zones (setup of src/minc.F90:58-374): the zone's cells become fracture cells with
        # nested matrix cells behind them
        self._order = None
        if minc_in and self._rock_controls:
            raise NotImplementedError("rock table controls together with MINC zones")
        if minc_in:
            from . import mesh as M
            by_name = {rt.get("name", "").strip(): rt for rt in rock.get("types", []) or []}
            zlist = []
            for mz in minc_in:
                fv = _get(mz, "geometry.fracture.volume")
                mv = list(np.atleast_1d(_get(mz, "geometry.matrix.volume", [0.9])))
                fv = 1.0 - sum(mv) if fv is None else fv
                planes = _get(mz, "geometry.fracture.planes", 1)
                spc = _get(mz, "geometry.fracture.spacing", 50.0)
                spc = [float(spc)] * planes if np.isscalar(spc) else (list(spc) + [spc[0]] * planes)[:planes]
                geo = M.MincGeometry([fv] + mv, spc, _get(mz, "geometry.fracture.connection", 0.0))
                rk = mz.get("rock", {}) or {}
                if isinstance(rk, list):
                    raise NotImplementedError("several rock specifications in one MINC zone")
                sel = []
                if rk.get("zones") is not None:
                    for zn in ([rk["zones"]] if isinstance(rk["zones"], str) else rk["zones"]):
                        sel.append(zone_cells(zones[zn], cen))
                if rk.get("types") is not None:
                    for tn in ([rk["types"]] if isinstance(rk["types"], str) else rk["types"]):
                        rt = by_name[tn.strip()]
                        if rt.get("cells") is not None:
                            sel.append(np.asarray(rt["cells"], dtype=int))
                        for zn in ([rt["zones"]] if isinstance(rt.get("zones"), str) else rt.get("zones") or []):
                            sel.append(zone_cells(zones[zn], cen))
                zc = np.unique(np.concatenate(sel)) if sel else np.arange(n)

                def named(key):
                    tn = _get(rk, key + ".type")
                    return rock_record(by_name[tn.strip()], dim) if tn is not None else None
                mrock = named("matrix")
                if mrock is None:
                    raise NotImplementedError("MINC matrix rock given by properties instead of a rock type")
                zlist.append(dict(cells=zc, geometry=geo, matrix_rock=mrock, fracture_rock=named("fracture")))
            lm = M.add_minc_zones(lm, zlist)
            self._order = lm.extras["waiwera_order"]
        self.owned_gid = np.arange(lm.n_owned)
        self._src_pick = None
        if self.cell_order_choice is None:      # the whole mesh as built, before its cells are dealt out to ranks
            fc = np.asarray(lm.face_cells if lm.face_cells is not None else [], dtype=np.int64).reshape(-1, 2)
            sp =np.asarray(lm.sub_ptr if lm.sub_ptr is not None else [0, lm.n_owned])
            share = _cut_share(fc[(fc < lm.n_owned).all(axis=1)], sp)
            self.cell_order_choice = CellOrderChoice("input", len(sp) - 1, int(np.diff(sp).max()) if len(sp) > 1 else 0, share, share)
        # what the initial conditions below need of the whole MINC mesh: its cell count, each cell's original cell and the
        # reference's cell order (on N ranks self._order becomes the rank's own)
        minc_all = (lm.n_owned, lm.extras["minc_parent"], self._order) if self._order is not None else None
        self._cell_index = None     # several ranks: the input's cell number -> the cell's place in the one-rank mesh
        if self.world > 1:
            if _get(inp, "time.step.adapt.method", "iteration") == "change":
                # (Timestepper._relative_change takes its maximum over the rank's own cells: the ranks would choose
                # different step sizes and part ways.  The same on every rank, before anything collective)
                raise NotImplementedError("step size adaption by the 'change' monitor on N ranks")
            from .partition import family_owner, partition_mesh
            # the owner of every cell, MINC families whole (each matrix cell with its fracture cell, family_owner)
            own = family_owner(lm, self.world, owner)
            if self._order is not None:
                self._cell_index = np.asarray(lm.extras["fracture_index"])
            # what the output file takes from the whole mesh, which every rank has built anyway: sizes, the faces' cells and
            # areas, MINC level and parent in the output's order.  Not gathered (_gathered_fields)
            wo = self._order
            self._whole = dict(
                n_cells=lm.n_owned, n_bc=lm.n_bc, n_faces=lm.n_faces, face_cells=np.asarray(lm.face_cells).reshape(-1, 2).copy(),
                face_area=np.asarray(lm.face_geom).reshape(-1, 12)[:, 0].copy(),
                bc_spec=np.asarray(lm.extras.get("bc_spec", np.zeros(lm.n_bc, dtype=np.int64))),
                minc=None if wo is None else (np.asarray(lm.extras["minc_level"])[wo], np.asarray(lm.extras["minc_parent"])[wo]))
            lm, self._gid = partition_mesh(lm, own, self.rank, world=self.world)
            # owned_gid: the rank's cells as the one-rank run's output numbers them -- the input's numbering; on a MINC mesh
            # the reference's order (the input's cells, then the matrix cells level by level), in which fields() lists them
            self.owned_gid = lm.owned_gid
            if self._order is not None:
                self._order, self.owned_gid = lm.extras["waiwera_order"], lm.extras["waiwera_gid"]
            # the place of every owned cell, in the rank's own (storage) order, in the one-rank output: what the gathers are keyed by
            self._cell_place = np.empty(lm.n_owned, dtype=np.int32)
            self._cell_place[np.arange(lm.n_owned) if self._order is None else self._order] = self.owned_gid
            # everything per source goes through _src_pick: the rank's sources as their numbers in the input, in the rank's order
            self._src_pick = lm.extras.get("src_global_index", np.zeros(0, dtype=np.int32))
            self._tables = self._pick_sources(self._tables)
            # rock table controls: the controlled cells this rank holds, ghosts included -- the permeability of a face
            # between two ranks reads the rock of both its cells
            self._rock_controls = [(fields, np.nonzero(np.isin(self._gid, cells))[0].astype(np.int32), tab)
                                   for fields, cells, tab in self._rock_controls]
        self.mesh = lm
        self.relperm = relperm_spec(rock.get("relative_permeability"))
        self.capillary = capillary_spec(rock.get("capillary_pressure"))
        # initial conditions
        init = inp.get("initial", {}) or {}
        npv = {"w": 1, "we": 2, "wce": 3, "wse": 3, "wae": 3, "wsce": 4, "wsae": 4}[self.eos]
        if "filename" in init:
            # restart from a Waiwera HDF5 output (setup_initial, src/initial.F90:421-677, 776, 922):
            # primaries of each cell from its fluid fields by region (eos%primary_variables)
            from . import hdf5io
            st = hdf5io.read_state(os.path.join(base_dir, init["filename"]), init.get("index", -1))
            region = np.rint(st["fluid_region"]).astype(np.int32) if "fluid_region" in st else np.ones(n, dtype=np.int32)
            cols = [st["fluid_pressure"]]
            if npv > 1:
                cols.append(np.where(region == 4, st["fluid_vapour_saturation"], st["fluid_temperature"]))
            if npv > 3:
                raise NotImplementedError("restart files for eos %s" % self.eos)
            if npv > 2 and self.eos == "wse":
                halite = np.isin(region, (5, 6, 8))
                cols[1] = np.where(np.isin(region, (4, 8)), st["fluid_vapour_saturation"], st["fluid_temperature"])
                cols.append(np.where(halite, st["fluid_solid_saturation"], st["fluid_liquid_salt_mass_fraction"]))
            elif npv > 2:
                cols.append(st["fluid_CO2_partial_pressure" if self.eos == "wce" else "fluid_air_partial_pressure"])
            prim = np.stack(cols, axis=1)
            if self._perm is not None and prim.shape[0] == n:      # read_state lists the file's cells by their /cell_index
                prim, region = prim[self._perm], region[self._perm]
            if prim.shape[0] != n and not (minc_all is not None and prim.shape[0] == minc_all[0]):
                raise ValueError("initial conditions file has %d cells, mesh has %d" % (prim.shape[0], n))
        else:
            prim = np.asarray(init.get("primary", [1.0e5, 20.0, 0.0][:npv]), dtype=np.float64)
            prim = np.tile(prim, (n, 1)) if prim.ndim == 1 else prim
            region = np.asarray(init.get("region", 1))
            region = np.full(n, int(region), dtype=np.int32) if region.ndim == 0 else region.astype(np.int32)
        if minc_all is not None:
            # matrix cells start from their fracture cell's state (src/initial.F90: MINC cells copy
            # the original cell's values unless the file holds them); file order = reference order.
            # On the WHOLE mesh, for either kind of initial conditions: the rank's share is cut out below
            nt, parent_all, order_all = minc_all
            src = np.empty(nt, dtype=np.int64)
            if prim.shape[0] == nt:        # restart file of a MINC run: already one record per cell
                src[order_all] = np.arange(nt)
            else:
                src[:] = parent_all
            prim, region = prim[src], region[src]
        if self.world > 1:
            prim, region = prim[self._gid], region[self._gid]
        self.primary, self.region = prim, region
        # the flow object
        tiles = None
        if self.subdomains == "rank":
            tiles = None if lm.sub_ptr is None else np.asarray(lm.sub_ptr, dtype=np.int32).copy()
            lm.sub_ptr = None       # one block per rank
            self.subdomain_choice = ("rank", "one block per rank, %s" % ("no tiles: the mesh has no chunks" if tiles is None
                                                                         else "tiles: the rank's %d chunks" % (tiles.size - 1)))
        else:
            self.subdomain_choice = ("chunks", "the mesh's chunks" if lm.sub_ptr is not None else "the mesh has no chunks: one block per rank")
        if ode_factory is None:
            from .flow_simulation import FlowSimulation
            self.ode = FlowSimulation(lm, eos=self.eos, device=device, temperature=temperature,
                                      relperm=self.relperm, capillary=self.capillary, thermo=self.thermo,
                                      permeability_modifier=self.permeability_modifier, thermo_extrapolate=self.thermo_extrapolate)
        elif self.thermo_extrapolate:
            # (an ode_factory evaluates the boundary fluid when it makes the object: the bound has to be part of that call)
            self.ode = ode_factory(lm, self.eos, self.thermo, self.relperm, self.capillary, temperature,
                                   permeability_modifier=self.permeability_modifier, thermo_extrapolate=True)
        elif self.permeability_modifier is not None:
            self.ode = ode_factory(lm, self.eos, self.thermo, self.relperm, self.capillary, temperature,
                                   permeability_modifier=self.permeability_modifier)
        else:
            self.ode = ode_factory(lm, self.eos, self.thermo, self.relperm, self.capillary, temperature)
        if tiles is not None:
            self.ode.set_pc_tiles(tiles)
        self.ode.set_regions(region)
        if any(self._production_components):      # the rank's own sources, in the rank's order (like owned_source below)
            pc = self._production_components
            self.ode.set_source_production_component(pc if self._src_pick is None else [pc[i] for i in self._src_pick])
        if self.world > 1:
            if comm_id is None:
                raise ValueError("several ranks need the communicator id of rank 0 (waiwera_amd.lib.comm_unique_id)")
            self.ode.comm_init(self.rank, self.world, comm_id)
        self.y = np.ascontiguousarray(self.ode.scale(prim, region).ravel())
        # solver and time stepping parameters
        step = _get(inp, "time.step", {}) or {}
        nl = _get(step, "solver.nonlinear", {}) or {}
        opts = {}
        if _get(nl, "tolerance.function.relative") is not None:
            opts["ftol_rel"] = nl["tolerance"]["function"]["relative"]
        if _get(nl, "tolerance.function.absolute") is not None:
            opts["ftol_abs"] = nl["tolerance"]["function"]["absolute"]
        if _get(nl, "maximum.iterations") is not None:
            opts["max_newton_its"] = nl["maximum"]["iterations"]
        if _get(nl, "minimum.iterations") is not None:
            opts["min_newton_its"] = nl["minimum"]["iterations"]
        # the flow solver: "time.step.solver.linear" (linear_solver_options).
        # An input that names no preconditioner gets the REFERENCE's default, restricted PCASM with overlap 1 over ILU(0)
        # (default_flow_pc_type_str = "asm", src/timestepper.F90:2019-2020) -- not the library's own default
        # (wai_default_opts: brick block Jacobi, the fused fast path).  Measured on the 216^3 bench system (round 6,
        # profiles/pc_compare_r6.log): asm 74 Krylov iterations at 7.83 ms, bjacobi 98 at 1.39 ms; a host that wants the
        # fast path for an unmodified input passes default_pc="bjacobi".  pc_choice records what was taken and why.
        lso = linear_solver_options(_get(step, "solver.linear"), self.default_pc, self.sub_lu)
        opts.update(lso["opts"])
        self.pc_choice = (lso["pc"], "input" if lso["named"] else ("reference default" if self.default_pc == "asm" else "default_pc argument")) + lso["note"]
        if opts:
            self.ode.set_opts(**opts)
        if lso["sub_device"]:
            self.ode.set_sub_pc("lu")
        if self.pc_ordering == "multicolour":
            net = self.inp.get("network") or {}
            refusal = pc_ordering_refusal(lso, bool(net.get("group") or net.get("reinject")))
            if refusal:
                raise NotImplementedError(refusal)
            self.ode.set_pc_ordering("multicolour")
            self.pc_choice += ("multicolour ordering of the blocks' ILU(0) (wai_set_pc_ordering)",)
        if self.pc_coarse is not None:
            net = self.inp.get("network") or {}
            refusal = pc_coarse_refusal(lso, bool(net.get("group") or net.get("reinject")), self.world, bool(self.inp.get("tracer")),
                                        self.pc_ordering == "multicolour")
            if refusal:
                raise NotImplementedError(refusal)
            self.ode.set_pc_coarse(self.pc_coarse, aggregates=coarse_aggregates_of(lm, self.coarse_aggregates))
            self.pc_choice += ("coarse level %s over %d aggregates (wai_set_pc_coarse)" % self.ode.pc_coarse(),)
        self._pc_covers_coupled = covers_coupled(lso)
        # the auxiliary (tracer) solver: "time.step.solver.auxiliary", the same keys (src/timestepper.F90:2057-2065).  The
        # reference's defaults for it are gmres and bjacobi (:2021-2022) whatever the flow solver uses; the library's tracer
        # solves FOLLOW the flow solver's preconditioner until told otherwise (wai_set_aux_pc), and an input without the
        # object keeps that -- no earlier result moves -- unless default_aux_pc asks for the reference's.  aux_pc_choice
        # records what was taken and why, like pc_choice
        aux_in = _get(step, "solver.auxiliary")
        if aux_in is None and self.default_aux_pc is None:
            self.aux_pc_choice = ("follow", "no auxiliary object: the flow solver's preconditioner (%s)" % self.pc_choice[0])
            self._aux_ilu_levels = opts.get("ilu_levels")
        else:
            als = linear_solver_options(aux_in, self.default_aux_pc or AUXILIARY_DEFAULT_PC, self.sub_lu, AUXILIARY_DEFAULTS)
            ao = als["opts"]
            why = "input" if als["named"] else ("reference default" if (self.default_aux_pc or AUXILIARY_DEFAULT_PC) == AUXILIARY_DEFAULT_PC
                                                else "default_aux_pc argument")
            self.aux_pc_choice = (als["pc"], why) + als["note"]
            self.ode.set_aux_solver(ao["ksp_type"], ao.get("gmres_restart", 30), ao["ksp_rtol"], 1e-50, ao.get("ksp_max_its", 10000))
            self.ode.set_aux_pc(ao["pc_type"], 1, ao.get("ilu_levels", 0), "lu" if als["sub_device"] else "ilu")
            self._pc_covers_coupled = covers_coupled(als)
            self._aux_ilu_levels = ao.get("ilu_levels")
        # tracers
        tr = inp.get("tracer")
        self.tracer_names = []
        self.X = None
        if tr:
            tr = tr if isinstance(tr, list) else [tr]
            phases = [{"liquid": 0, "vapour": 1}[t.get("phase", "liquid")] for t in tr]
            self.tracer_names = [t.get("name", "tracer") for t in tr]
            nt = len(tr)

            def tvals(v):
                v = 0.0 if v is None else v
                return [v] * nt if np.isscalar(v) else list(v)
            bc = np.array([tvals(b.get("tracer")) for b in inp.get("boundaries", []) or []
                           for f in (b["faces"] if isinstance(b["faces"], list) else [b["faces"]]) for _ in f["cells"]])
            # tracer injection rates: numbers, or [[t, q], ...] tables averaged over each step interval
            # like the rate tables (tracer table source controls, src/source_setup.F90:2415-2560)
            self._tracer_tables, rows = [], []
            for i, s in enumerate(inp.get("source", []) or []):
                v = s.get("tracer")
                if isinstance(v, (list, tuple)) and v and isinstance(v[0], (list, tuple)):
                    if nt != 1:
                        raise NotImplementedError("tracer injection tables with several tracers")
                    tab = Table(v, s.get("interpolation", "linear"), s.get("averaging", "integrate"))
                    self._tracer_tables.append((i, 0, tab))
                    v = float(tab.interpolate(_get(inp, "time.start", 0.0))[0])
                rows.append(tvals(v))
            inj = np.array(rows) if srcs else None
            if self.world > 1:
                # the rank's share: boundary values of its boundary cells, injection rows and tables of its sources.  (The
                # initial value is one number per tracer: nothing to cut.)  None of this is collective; a rank without
                # tracer source or boundary still makes every assembly and solve call, the time stepper's (Timestepper.step)
                if lm.n_bc:
                    bc = bc[lm.extras["bc_global_index"]]
                inj = inj[self._src_pick] if srcs and len(self._src_pick) else None
                self._tracer_tables = self._pick_sources(self._tracer_tables)
            self._tracer_injection = inj
            self.ode.set_tracers(phases, decay=[t.get("decay", 0.0) for t in tr],
                                 activation=[t.get("activation", 0.0) for t in tr],
                                 diffusion=[t.get("diffusion", 0.0) for t in tr],
                                 bc=bc if lm.n_bc else None, injection=inj)
            self.X = np.tile(np.asarray(tvals(init.get("tracer")), dtype=np.float64), lm.n_owned)
            if self.tracer_solve == "coupled" and nt > 1 and not self._pc_covers_coupled:
                # (one tracer takes the per-tracer path in either mode: nothing to refuse.  Decided on the input and the
                # arguments alone, before the first collective call after comm_init: every rank raises, none waits)
                if self.aux_pc_choice[0] == "follow":
                    raise ValueError("tracer_solve='coupled' covers the bjacobi (ILU(0)) and none preconditioners; this run's is %r (%s)"
                                     "%s: pass default_pc='bjacobi' or tracer_solve='per_tracer'"
                                     % (self.pc_choice[0], self.pc_choice[1], " with ILU(k)" if opts.get("ilu_levels") else ""))
                raise ValueError("tracer_solve='coupled' covers the bjacobi (ILU(0)) and none preconditioners; this run's auxiliary "
                                 "preconditioner is %r (%s)%s: pass tracer_solve='per_tracer', or name 'bjacobi' in the auxiliary solver object"
                                 % (self.aux_pc_choice[0], self.aux_pc_choice[1], " with ILU(k)" if self._aux_ilu_levels else ""))
        ad = step.get("adapt", {}) or {}
        mx = step.get("maximum", {}) or {}
        self.ts = Timestepper(
            self.ode, self.y, time=_get(inp, "time.start", 0.0), stepsize=step.get("size", 0.1),
            method=step.get("method", "beuler"), adapt=bool(ad.get("on", False)),
            adapt_method=ad.get("method", "iteration"), adapt_min=ad.get("minimum", 5.0),
            adapt_max=ad.get("maximum", 8.0), reduction=ad.get("reduction", 0.2),
            amplification=ad.get("amplification", 2.0), max_stepsize=mx.get("size") or 0.0,
            max_num_tries=_get(step, "maximum.tries", 10), stop_time=_get(inp, "time.stop"),
            max_num_steps=mx.get("number") if mx.get("number") is not None else 100, aux_solution=self.X,
            checkpoints=_get(inp, "output.checkpoint.time"),
            checkpoint_tolerance=_get(inp, "output.checkpoint.tolerance", 0.1),
            tracer_solve_mode=self.tracer_solve if self.tracer_solve != "per_tracer" else None)
        if _get(inp, "output.checkpoint.repeat") not in (None, False, 1):
            raise NotImplementedError("repeated output checkpoints")

        src_in = inp.get("source", []) or []
        # On several ranks the initial fluid state some controls need (reference pressure "initial", productivity index
        # from the initial rate) comes out of a pre_eval, and a pre_eval there exchanges halos: it is made on EVERY rank,
        # decided on the unfiltered source list -- a rank without such a source would otherwise never issue the matching
        # exchange (advisor, round 5)
        need_fluid = self.world > 1 and any(k in s_ for s_ in src_in for k in ("deliverability", "recharge", "injectivity"))
        # the sources as the input numbers them, for the rank's own: fields()["source_*"] and save()'s owned_source
        self.owned_source = np.arange(len(src_in)) if self._src_pick is None else np.asarray(self._src_pick, dtype=np.int64)
        if self._src_pick is not None:      # the sources of this rank's cells, in the rank's order
            src_in = [src_in[i] for i in self._src_pick]
        self._setup_source_controls(src_in, _get(inp, "time.start", 0.0), collective_fluid=need_fluid)
        self._setup_network(inp)
        if (self._tables or self._ctl_tables or getattr(self, "_tracer_tables", None) or getattr(self, "_network_timed", False)
                or self._rock_controls):
            # (decided on what the INPUT holds, not on this rank's share, where a control is collective: _network_timed)
            self.ts.controls = self._update_controls

    # ---- source network --------------------------------------------------------------------------
    def _setup_network(self, inp):
        """"network": {"group": [...], "reinject": [...]} handed to wai_set_source_network; descriptions
        with time tables are sent again for every step interval (_update_controls)"""
        t0 = _get(inp, "time.start", 0.0)
        spec, names, timed = network_spec(inp, (t0, t0), self.ode.separator_enthalpies if hasattr(self.ode, "separator_enthalpies") else None)
        self.network_names = names
        self._network_timed = timed
        if spec is not None:
            if self.world > 1:
                # EVERY rank holds the whole network (the reference broadcasts the JSON too), its sources numbered as in the
                # input; the library is told which of them are this rank's.  set_source_network is collective there (the
                # separators and injection enthalpies of all ranks' sources are gathered): made on every rank, with or
                # without a source of the network -- `spec` depends on the input alone
                self.ode.set_source_global_index(len(inp.get("source", []) or []), self._src_pick)
            self.ode.set_source_network(spec)
            if self.network_walk == "wave":      # (before the pass' place is read back: the wave walk holds larger networks)
                self.ode.set_network_walk("wave")
            if self.network_pass == "device":
                self.ode.set_network_pass("device")
                self.network_pass_choice = self.ode.network_pass()
            if self.coupling_build == "batched":
                self.ode.set_coupling_build("batched")
                self.coupling_build_choice = self.ode.coupling_build()
            if self.network_walk == "wave":
                self.network_walk_choice = self.ode.network_walk()

    # ---- state-dependent source controls -------------------------------------------------------
    def _setup_source_controls(self, sources, t0, collective_fluid=False):
        """Deliverability, recharge, limiter, separator and direction of each source
        (setup_inline_source_controls, src/source_setup.F90:2340-2412) as the control records the
        device evaluates (include/waiwera_hip.h, wai_source_control); their time tables are kept
        here and averaged over every step interval (_update_controls)"""
        self._ctl, self._ctl_tables = None, []
        fl = None
        if collective_fluid:      # every rank together, whether or not it owns such a source
            self._pre_eval(t0)
            fl = np.asarray(self.ode.fluid())
        if not any(k in s for s in sources for k in ("deliverability", "recharge", "injectivity", "limiter",
                                                     "direction", "factor", "separator")):
            return
        recs = [dict() for _ in sources]

        def timed(v, default, s):     # number | [[t, v], ...] | {"time": [[t, v], ...]} -> Table
            if isinstance(v, dict):
                v = v.get("time")
            if v is None:
                v = default
            data = v if isinstance(v, (list, tuple)) else [[0.0, float(v)]]
            return Table(data, s.get("interpolation", "linear"), s.get("averaging", "integrate"))

        def cell_fluid(cell):
            nonlocal fl
            if fl is None:
                if self.world > 1:
                    raise RuntimeError("initial fluid state asked for on one rank only: the evaluation is collective")
                self._pre_eval(t0)
                fl = np.asarray(self.ode.fluid())
            if self.world > 1:      # the input's cell number -> this rank's (the source is on this rank: its cell is owned)
                if self._cell_index is not None:      # a MINC mesh keeps the input's cells elsewhere
                    cell = int(self._cell_index[cell])
                cell = int(np.nonzero(self.mesh.owned_gid == cell)[0][0])
            return fl[cell]

        nc = {"w": 1, "we": 1, "wce": 2, "wse": 2, "wae": 2, "wsce": 3, "wsae": 3}[self.eos]
        f0, pd = 6 + nc, 7 + nc

        def mobility_sum(f):
            phases = int(round(f[4]))
            return sum(f[f0 + p * pd + 3] * f[f0 + p * pd] / f[f0 + p * pd + 1] for p in range(2) if phases & (1 << p))

        for i, s in enumerate(sources):
            r = recs[i]
            for key, kind, cdef, ckey in (("deliverability", "deliverability", 1.0e-11, "productivity"),
                                          ("recharge", "recharge", 0.0, "coefficient"),
                                          ("injectivity", "recharge", 0.0, "coefficient")):   # same control, :3013
                if key not in s:
                    continue
                spec = s[key] if isinstance(s[key], dict) else {}
                thr = float(spec.get("threshold", -1.0) or -1.0)
                if thr > 0.0:
                    # deliverability that switches on below a threshold pressure (source_control.F90:99-100, 489-503;
                    # source_setup.F90:2855-2911): the source keeps its own rate above it
                    if kind != "deliverability":
                        raise ValueError("threshold belongs to a deliverability control")
                    r["threshold"] = thr
                r["kind"] = kind
                pr = spec.get("pressure", 1.0e5)
                if isinstance(pr, str):
                    if pr.lower() != "initial":
                        raise ValueError("reference pressure %r" % pr)
                    pr = float(cell_fluid(s["cell"])[0])      # set_reference_pressure_initial
                if isinstance(pr, dict) and ("enthalpy" in pr or "pressure" in pr):
                    if kind != "deliverability" or s.get("interpolation", "linear") != "linear":
                        raise NotImplementedError("reference pressure table against enthalpy / pressure")
                    r["table_coord"] = "enthalpy" if "enthalpy" in pr else "pressure"
                    r["table"] = [tuple(q) for q in pr[r["table_coord"]]]
                else:
                    self._ctl_tables.append((i, "pressure", timed(pr, 1.0e5, s)))
                if ckey in spec or kind == "recharge" or "rate" not in s or thr > 0.0:
                    self._ctl_tables.append((i, "coef", timed(spec.get(ckey), cdef, s)))
                    if thr > 0.0:   # threshold_productivity starts as the productivity at the start time (:2906-2909)
                        r["threshold_pi"] = float(self._ctl_tables[-1][2].interpolate(t0)[0])
                else:
                    # productivity index from the initial rate (calculate_PI_from_rate,
                    # src/source_control.F90:407-468) on the initial fluid
                    f = cell_fluid(s["cell"])
                    pref = r["table"][0][1] if "table" in r else self._ctl_tables[-1][2].interpolate(t0)[0]
                    factor = mobility_sum(f) * (f[0] - pref)
                    r["coef"] = abs(s["rate"]) / factor if abs(factor) > 1.0e-9 else cdef
            if "limiter" in s:
                lim = s["limiter"]
                if "limit" not in lim and "type" not in lim:
                    kinds = [k for k in ("total", "water", "steam") if k in lim]
                    if len(kinds) != 1:
                        raise NotImplementedError("limiters on several flow types")
                    lim = dict(lim, type=kinds[0], limit=lim[kinds[0]])    # {"total": 2.0} form
                r["limiter"] = lim.get("type", "total")
                ls = dict(s, **{k: lim[k] for k in ("interpolation", "averaging") if k in lim})
                self._ctl_tables.append((i, "limit", timed(lim.get("limit"), 1.0, ls)))
            sep = s.get("separator")
            psep = None
            if sep is not None and sep is not False:
                psep = sep.get("pressure", 0.55e6) if isinstance(sep, dict) else 0.55e6
            elif "limiter" in s and "separator_pressure" in s["limiter"]:
                psep = s["limiter"]["separator_pressure"]
            stages = list(psep) if isinstance(psep, (list, tuple)) else [psep]
            if len(stages) > 4:
                raise NotImplementedError("separators with more than 4 stages")
            has_sep = psep is not None and stages and all(p is not None and p > 0.0 for p in stages)   # separator_init, separator.F90:182
            if has_sep:     # also what the source network separates the source's flow with
                r["sep_hf"], r["sep_hg"] = self.ode.separator_enthalpies(float(stages[0]))
                r["sep_more"] = [self.ode.separator_enthalpies(float(p)) for p in stages[1:]]
            elif r.get("limiter") in ("water", "steam"):
                r["limiter"] = None      # no separator: separated flows are zero, never over the limit
            if "direction" in s:
                r["direction"] = s["direction"].lower()
            if "factor" in s:      # rate factor, applied after every other control (:2615-2660)
                fac = s["factor"]
                fs = dict(s)
                if isinstance(fac, dict):
                    fs.update({k: fac[k] for k in ("interpolation", "averaging") if k in fac})
                self._ctl_tables.append((i, "factor", timed(fac, 1.0, fs)))
        self._ctl = recs
        self._apply_controls((t0, t0))
        for r in self._ctl:
            r.pop("threshold_pi", None)     # from now on the index the device notes (wai_set_source_controls keeps it)

    def _pre_eval(self, t):
        """the fluid state of self.y (a halo exchange on N ranks: collective).  Not inside an assert: python -O would
        take the call away with the check"""
        rc = self.ode.pre_eval(t, self.y)
        if rc != 0:
            raise RuntimeError("the fluid state at t = %g could not be evaluated (pre_eval returned %d)" % (t, rc))

    def _pick_sources(self, entries):
        """(source, ...) entries numbered as in the input -> those of this rank's sources, numbered as the rank holds them"""
        local = {int(g): i for i, g in enumerate(self._src_pick)}
        return [(local[e[0]],) + tuple(e[1:]) for e in entries if e[0] in local]

    def _apply_controls(self, interval):
        for i, key, tab in self._ctl_tables:
            self._ctl[i][key] = float(tab.average(interval)[0])
        self.ode.set_source_controls(self._ctl)

    def _update_controls(self, interval):
        """table_object_control_update (src/control.F90:263-284): each table's average over the step
        interval becomes the rate / enthalpy of its source; likewise the productivity, reference
        pressure and limit tables of the state-dependent controls"""
        # rock controls: flow_simulation_pre_try_timestep(t) with t the time the try ends at (timestepper.F90:2333),
        # the table's value AT that time (rock_control.F90:66, 102: interpolate, not an interval average); a scalar
        # permeability fills all directions
        # (wai_update_rock copies one plane of the rock record to the host and back: nothing in it is collective.  Every
        # rank still makes the call, with the cells it holds -- none, for a rank without the rock type)
        for fields, cells, tab in self._rock_controls:
            v = tab.interpolate(float(interval[1]))
            for q, f in enumerate(fields):
                self.ode.update_rock(f, cells, v[0] if tab.dim == 1 else v[min(q, tab.dim - 1)])
        if self._tables:
            rate, enth = self.mesh.src_rate.copy(), self.mesh.src_enthalpy.copy()
            for i, key, tab in self._tables:
                (rate if key == "rate" else enth)[i] = tab.average(interval)[0]
            self.ode.set_source_rates(rate, enth)
        if self._ctl_tables:
            self._apply_controls(interval)
        if getattr(self, "_network_timed", False):
            spec, _, _ = network_spec(self.inp, interval, self.ode.separator_enthalpies)
            self.ode.set_source_network(spec)
        if getattr(self, "_tracer_tables", None):
            for i, it, tab in self._tracer_tables:
                self._tracer_injection[i, it] = tab.average(interval)[0]
            self.ode.set_tracer_injection(self._tracer_injection)

    @classmethod
    def from_json(cls, path, **kw):
        with open(path) as f:
            inp = json.load(f)
        return cls(inp, base_dir=os.path.dirname(os.path.abspath(path)), **kw)

    def run(self):
        """timestepper_run with the output schedule of "output" (initial / frequency / final,
        src/timestepper.F90:2478-2560); returns the final cell fields under the reference's names
        and, if "output.filename" is given (and the HDF5 library is there), writes that file -- on several ranks rank 0
        does, from snapshots gathered through the library (the returned fields stay the rank's own)"""
        self._pre_eval(self.ts.time)
        if self.X is not None:
            self.ts.init_auxiliary()
        oc = self.inp.get("output")
        oc = {} if oc in (None, True) else ({"frequency": 0, "initial": False, "final": False} if oc is False else oc)
        freq, self.outputs = oc.get("frequency", 1), []
        # Several ranks and an output file: every snapshot is a collective gather to rank 0 (_gathered_fields), which keeps the
        # list and writes the file; the other ranks keep nothing.  Whether a snapshot is taken depends on the input and the
        # step history alone, the same on every rank -- never on what a rank holds or on whether its HDF5 library loads
        gathered = self._gathered = self.world > 1 and bool(oc.get("filename"))

        def snapshot():
            f = self._gathered_fields() if gathered else self.fields()
            if f is not None:
                self.outputs.append(f)
        if oc.get("initial", True):
            snapshot()
        try:
            while not self.ts.finished:
                self.ts.step()
                hit = self.ts.checkpoint_hit
                if hit or (freq and self.ts.taken % freq == 0) or (self.ts.finished and oc.get("final", True)):
                    snapshot()
                if hit:
                    self.ts.checkpoint_update()
        finally:
            # the reference keeps what it has written when a step aborts; a file that cannot be written
            # is reported, not swallowed (the results are still returned).  Several ranks: rank 0 holds the snapshots
            if oc.get("filename") and self.outputs and (self.world == 1 or self.rank == 0):
                try:
                    self.save_hdf5(os.path.join(self.output_dir, oc["filename"]))
                except Exception as e:
                    self.output_error = e
                    import sys
                    print("waiwera_amd: output file %r not written: %s" % (oc["filename"], e), file=sys.stderr)
        return self.fields()

    def datasets(self):
        """{HDF5 path: array} of the collected snapshots (output_datasets), or of the state in force when there are none.
        Several ranks: the snapshots gathered on rank 0 by a run with "output.filename"; None on a rank that holds none"""
        outs = getattr(self, "outputs", None)
        if self.world > 1:
            if not outs or not getattr(self, "_gathered", False):
                return None
            minc = self._whole["minc"]
            return output_datasets(outs, self._whole["n_cells"], *(minc or ()))
        outs = outs or [self.fields()]
        if self._order is None:
            return output_datasets(outs, self.mesh.n_owned)
        ex = self.mesh.extras
        return output_datasets(outs, self.mesh.n_owned, np.asarray(ex["minc_level"])[self._order], np.asarray(ex["minc_parent"])[self._order])

    def save_hdf5(self, path):
        """the collected outputs in the reference's layout (output_datasets) written through waiwera_amd.hdf5io"""
        from . import hdf5io
        data = self.datasets()
        if data is None:
            raise RuntimeError("no gathered snapshots on rank %d of %d: run() with \"output.filename\" collects them on rank 0" % (self.rank, self.world))
        hdf5io.write_file(path, data)

    def _fluid_columns(self):
        """[(output field, column of the fluid record)] of the cell fields taken from the fluid vector, in fields()' order"""
        nc = {"w": 1, "we": 1, "wce": 2, "wse": 2, "wae": 2, "wsce": 3, "wsae": 3}[self.eos]
        f0, pd = 6 + nc, 7 + nc
        cols = [("fluid_pressure", 0), ("fluid_temperature", 1), ("fluid_region", 2), ("fluid_liquid_saturation", f0 + 2),
                ("fluid_liquid_density", f0)]
        if self.eos != "w":
            cols += [("fluid_vapour_saturation", f0 + pd + 2), ("fluid_vapour_density", f0 + pd)]
        if self.eos in ("wse", "wsce", "wsae"):
            cols += [("fluid_liquid_salt_mass_fraction", f0 + 8), ("fluid_solid_saturation", f0 + 2 * pd + 2)]
        if self.eos in ("wsce", "wsae"):
            gas = "CO2" if self.eos == "wsce" else "air"
            cols += [("fluid_%s_partial_pressure" % gas, 8), ("fluid_liquid_%s_mass_fraction" % gas, f0 + 9),
                     ("fluid_vapour_%s_mass_fraction" % gas, f0 + pd + 9)]
        if self.eos in ("wce", "wae"):
            gas = "CO2" if self.eos == "wce" else "air"
            cols += [("fluid_%s_partial_pressure" % gas, 7), ("fluid_liquid_%s_mass_fraction" % gas, f0 + 8),
                     ("fluid_vapour_%s_mass_fraction" % gas, f0 + pd + 8)]
        return cols

    def _flux_names(self):
        """(names of the flux vector's columns, those "output.fields.flux" asks for) -- src/flow_simulation.F90:460-504"""
        oc = self.inp.get("output")
        want = ((oc.get("fields") if isinstance(oc, dict) else None) or {}).get("flux") or []
        comps = {"w": ["water"], "we": ["water", "energy"], "wce": ["water", "CO2", "energy"],
                 "wae": ["water", "air", "energy"], "wse": ["water", "salt", "energy"],
                 "wsce": ["water", "salt", "CO2", "energy"], "wsae": ["water", "salt", "air", "energy"]}[self.eos]
        names = comps + (["liquid"] if self.eos == "w" else ["liquid", "vapour"])
        return names, (names if want == "all" or "all" in want else list(want))

    def _gathered_fields(self):
        """One snapshot of a run on several ranks, gathered to rank 0 through the library (wai_gather_fluid,
        wai_gather_rows): fields() of the WHOLE mesh there, None on the other ranks.  COLLECTIVE: every rank makes every
        call below, in this order, whatever it holds -- each condition reads the input alone.
        Cell fields are keyed by the cells' places in the one-rank output, source fields by the sources' numbers in the
        input, flux fields by face_gid (each face from the rank that owns it, partition.face_owner; the sign turned where
        face_flip says the local orientation is reversed).  The network's nodes are the same on every rank and are taken
        from rank 0; cell indices, MINC levels, the faces' cells and areas come from the whole mesh (self._whole)."""
        ode, W, n, root = self.ode, self._whole, self.mesh.n_owned, self.rank == 0
        self.ode.pre_eval(self.ts.time, self.y)
        cols = self._fluid_columns()
        F = ode.gather_fluid([c for _, c in cols], self._cell_place, W["n_cells"])
        # geometry and tracers: host rows of the owned cells, in the rank's own order like the places
        geom = np.asarray(self.mesh.cell_geom)[:n]
        rows = [geom[:, : self.dim], geom[:, 3:4]] + ([self.X.reshape(n, -1)] if self.X is not None else [])
        G = ode.gather_rows(np.hstack(rows), self._cell_place, W["n_cells"])
        out = None
        if root:
            out = {"time": self.ts.time}
            for k, (name, _) in enumerate(cols[:5]):
                out[name] = F[:, k].copy()
            out["cell_geometry_centroid"], out["cell_geometry_volume"] = G[:, : self.dim].copy(), G[:, self.dim].copy()
            for k, (name, _) in enumerate(cols[5:]):
                out[name] = F[:, 5 + k].copy()
            for k, name in enumerate(self.tracer_names if self.X is not None else []):
                out["tracer_" + name] = G[:, self.dim + 1 + k].copy()
        oc = self.inp.get("output")
        want = (oc.get("fields") if isinstance(oc, dict) else None) or {}
        ns = len(self.inp.get("source", []) or [])
        together = bool(self.network_names["group"] or self.network_names["reinject"])
        sep_names = ("water_rate", "water_enthalpy", "steam_rate", "steam_enthalpy")
        src_want = want.get("source") or []
        if ns:      # the input has sources: every rank gathers, with the rows of its own -- none on a rank without
            names = ["source_rate", "source_enthalpy"]
            loc = list(ode.source_rates(together))
            if any(k in src_want for k in sep_names):
                sep = ode.source_separated(together)
                for j, k in enumerate(sep_names):
                    if k in src_want:
                        names.append("source_" + k)
                        loc.append(sep[:, j])
            S = ode.gather_rows(np.stack(loc, axis=1).reshape(self.mesh.n_src, len(names)), self.owned_source, ns)
            if root:
                out["source_rate"], out["source_enthalpy"] = S[:, 0].copy(), S[:, 1].copy()
        fnames, fwant = self._flux_names()
        if fwant:
            ex = self.mesh.extras
            own = np.asarray(ex["face_owned"], dtype=bool)
            fx = ode.fluxes()[:, [fnames.index(nm) for nm in fwant]]
            fx = np.where(np.asarray(ex["face_flip"], dtype=bool)[:, None], -fx, fx)[own]
            X = ode.gather_rows(fx.reshape(int(own.sum()), len(fwant)), np.asarray(ex["face_gid"])[own], W["n_faces"])
            if root:
                for k, nm in enumerate(fwant):
                    out["flux_" + nm] = X[:, k].copy()
                out["face_cell_1"], out["face_cell_2"], out["face_geometry_area"] = \
                    face_output(W["face_cells"], W["n_cells"], W["n_bc"], W["bc_spec"], W["face_area"])
        if root and ns:      # (the separated flows stand behind the face fields, as in fields())
            for k, name in enumerate(names[2:]):
                out[name] = S[:, 2 + k].copy()
        if root and together:
            out.update(self._network_fields(want))
        return out

    def _network_fields(self, want):
        """the source network's group and reinjector fields after the last pass"""
        out = {}
        G, R = self.ode.source_network()
        gcols = ("rate", "enthalpy", "water_rate", "water_enthalpy", "steam_rate", "steam_enthalpy")
        for k in (want.get("network_group") or []):
            if k in gcols and len(G):
                out["network_group_" + k] = G[:, gcols.index(k)].copy()
        rcols = ("output_water_rate", "output_steam_rate", "overflow_rate", "overflow_enthalpy", "overflow_water_rate",
                 "overflow_water_enthalpy", "overflow_steam_rate", "overflow_steam_enthalpy")
        for k in (want.get("network_reinject") or ["output_water_rate", "output_steam_rate", "overflow_water_rate",
                                                   "overflow_steam_rate"]):
            if k in rcols and len(R):
                out["network_reinject_" + k] = R[:, rcols.index(k)].copy()
        return out

    def fields(self):
        n = self.mesh.n_owned
        self.ode.pre_eval(self.ts.time, self.y)
        fl = np.asarray(self.ode.fluid())[:n]
        geom = self.mesh.cell_geom[:n]
        if self._order is not None:      # MINC: the reference's cell order (original cells, then level by level)
            fl, geom = fl[self._order], geom[self._order]
        if self._inv is not None:        # the compact cell order: back to the input's numbering
            fl, geom = fl[self._inv], geom[self._inv]
        cols = self._fluid_columns()
        out = {"time": self.ts.time}
        for name, col in cols[:5]:
            out[name] = fl[:, col].copy()
        out["cell_geometry_centroid"], out["cell_geometry_volume"] = geom[:, : self.dim].copy(), geom[:, 3].copy()
        for name, col in cols[5:]:
            out[name] = fl[:, col].copy()
        if self.X is not None:
            for k, name in enumerate(self.tracer_names):
                xk = self.X.reshape(n, -1)[:, k]
                back = self._order if self._order is not None else self._inv
                out["tracer_" + name] = (xk[back] if back is not None else xk).copy()
        # A source network on N ranks: reading the sources' rates runs the network pass, which gathers every rank's
        # sources -- a rank without any reads them too (`together`; decided on the input alone)
        together = self.world > 1 and bool(getattr(self, "network_names", None)) and \
            bool(self.network_names["group"] or self.network_names["reinject"])
        if (self.mesh.n_src or together) and hasattr(self.ode, "source_rates"):
            out["source_rate"], out["source_enthalpy"] = self.ode.source_rates(True) if together else self.ode.source_rates()
        oc = self.inp.get("output")
        want = (oc.get("fields") if isinstance(oc, dict) else None) or {}
        # face fields: "output.fields.flux" (src/flow_simulation.F90:460-504): the flux vector's
        # components and phases by name, per unit area, positive from face_cell_1 to face_cell_2
        names, flux_names = self._flux_names()
        if flux_names and hasattr(self.ode, "fluxes"):
            fx = self.ode.fluxes()
            face_cells, face_area = self.mesh.face_cells, np.asarray(self.mesh.face_geom)[:, 0]
            if self._input_faces is not None:
                # the compact cell order: the faces as the input-order mesh lists and orients them
                back, area = np.empty_like(fx), np.empty_like(face_area)
                back[self._face_place] = np.where(self._face_flip[:, None], -fx, fx)
                area[self._face_place] = face_area
                fx, face_cells, face_area = back, self._input_faces, area
            for nm in flux_names:
                out["flux_" + nm] = fx[:, names.index(nm)].copy()
            out["face_cell_1"], out["face_cell_2"], out["face_geometry_area"] = face_output(
                face_cells, self.mesh.n_owned + self.mesh.n_halo, self.mesh.n_bc,
                self.mesh.extras.get("bc_spec", np.zeros(self.mesh.n_bc, dtype=np.int64)), face_area)
        # separated water / steam flows of the sources and the source network's nodes
        src_want = want.get("source") or []
        if (self.mesh.n_src or together) and hasattr(self.ode, "source_separated") and \
                any(k in src_want for k in ("water_rate", "water_enthalpy", "steam_rate", "steam_enthalpy")):
            sep = self.ode.source_separated(True) if together else self.ode.source_separated()
            for j, k in enumerate(("water_rate", "water_enthalpy", "steam_rate", "steam_enthalpy")):
                if k in src_want:
                    out["source_" + k] = sep[:, j].copy()
        if getattr(self, "network_names", None) and hasattr(self.ode, "source_network") and \
                (self.network_names["group"] or self.network_names["reinject"]):
            out.update(self._network_fields(want))
        return out

    def save(self, path):
        np.savez(path, owned_gid=self.owned_gid, owned_source=self.owned_source, **self.fields())
