"""The source term of one cell with injection and production components, restated in numpy from the reference's definition
(source_update_flow and what it calls, src/source.F90:340-366 and 403-453; fluid%phase_flow_fractions,
%component_flow_fractions and %specific_enthalpy, src/fluid.F90:377-453) -- not from the device code.  Its input is the
device's own fluid record of the cell (wai_get_fluid: the reference's layout, src/fluid.F90:212-267), so that the comparison
holds the handful of products of the source term alone.

    rate > 0 (injection)   component = injection component, 1 where none is given; enthalpy = the injection enthalpy;
                           flow(component) = rate
    rate <= 0 (production) component = production component; where none is given (0) the injection component stands in, as
                           the library has it, 0 = all; for component < np the phase flow fractions and (not isothermal) the
                           flowing enthalpy are formed; component <= 0 spreads the rate over the mass components by their
                           flow fractions, any other puts all of it into flow(component)
    both                   component < np: flow(np) += enthalpy * rate.  component = np is heat alone.
"""
import numpy as np

NP = {"w": 1, "we": 2, "wce": 3, "wae": 3}
NC = {"w": 1, "we": 1, "wce": 2, "wae": 2}
NPH = {"w": 1, "we": 2, "wce": 2, "wae": 2}


def phase_fields(rec, eos):
    """per phase of a fluid record: (present, density, viscosity, relative permeability, specific enthalpy, mass fractions)"""
    nc = NC[eos]
    f0, pd = 6 + nc, 7 + nc
    phases = int(round(rec[4]))
    out = []
    for p in range(NPH[eos]):
        b = f0 + p * pd
        out.append((bool(phases & (1 << p)), rec[b], rec[b + 1], rec[b + 3], rec[b + 5], rec[b + 7: b + 7 + nc]))
    return out


def source_flow(rec, eos, rate, enthalpy, component, production_component):
    """(flow[np], enthalpy) of one source on the cell whose fluid record is rec"""
    np_, nc = NP[eos], NC[eos]
    isothermal = eos == "w"
    flow = np.zeros(np_)
    if rate > 0.0:
        c = 1 if component <= 0 else component
        h = enthalpy
        flow[c - 1] = rate
    else:
        c = production_component if production_component > 0 else max(component, 0)
        h = 0.0
        ph = phase_fields(rec, eos)
        if c < np_:
            mob = np.array([kr * rho / mu if on else 0.0 for on, rho, mu, kr, _, _ in ph])
            total = 0.0
            for m in mob:
                total += m
            frac = mob / total
            if not isothermal:
                for (on, _, _, _, hp, _), f in zip(ph, frac):
                    if on:
                        h += f * hp
        if c <= 0:
            cf = np.zeros(nc)
            for q in range(nc):
                for (on, _, _, _, _, x), f in zip(ph, frac):
                    if on:
                        cf[q] += f * x[q]
            cs = 0.0
            for v in cf:
                cs += v
            flow[:nc] = rate * (cf / cs)
        else:
            flow[c - 1] = rate
    if not isothermal and c < np_:
        flow[np_ - 1] += h * rate
    return flow, h


def source_rows(fluid, eos, volume, sources):
    """what the sources add to wai_rhs, [n_cells, np]: each source's flow over its cell's volume, added in input order.
    sources: [(cell, rate, enthalpy, component, production_component)]"""
    out = np.zeros((len(volume), NP[eos]))
    for cell, rate, enthalpy, comp, pcomp in sources:
        flow, _ = source_flow(fluid[cell], eos, rate, enthalpy, comp, pcomp)
        out[cell] += flow / volume[cell]
    return out
