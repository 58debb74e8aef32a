"""Times wai_residual and wai_jacobian with the source network's pass on the host (the default) and on the device
(wai_set_network_pass) in ONE process, the modes alternating: a host clock around `reps` calls that end in a device
synchronise, warm-ups first, `rounds` rounds per mode; the median over the rounds and their spread ((max - min) / median) per
mode -- the bar a difference between the modes has to clear.  Stream waits and passes per call come from the library's
own counters (wai_test_network_stats).

Cases: the reference's reinjection benchmark after three time steps (the case of tools/network_pass_cost.py), and a
synthetic 32 x 32 x 8 mesh with 8, 64 and 256 networked wells -- deliverability producers in two limited groups (one uniform,
one progressive) behind separators, whose water one reinjector shares out among the remaining wells, the last one taking
the overflow.  One JSON line per case:

    python tools/network_device_timing.py > profiles/network_device_timing.json
    python tools/network_device_timing.py --wells 8 --reps 20          # one synthetic size, quickly"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
MODES = ("host", "device")


def timed(ode, call, reps, warm):
    for _ in range(warm):
        call()
    ode.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    ode.synchronize()
    return 1.0e6 * (time.perf_counter() - t0) / reps


def measure(ode, y, dt, rounds, reps, jac_reps):
    n = ode.n_owned * ode.num_primary_variables
    f, lhs = np.zeros(n), np.zeros(n)
    assert ode.pre_eval(0.0, y) == 0
    ode.lhs(0.0, (0.0, 0.0), y, lhs)
    out = {m: dict(residual_us=[], jacobian_us=[]) for m in MODES}
    for _ in range(rounds):
        for m in MODES:
            ode.set_network_pass(m)
            assert ode.network_pass() == (m, m), ode.network_pass()
            row = out[m]
            row["residual_us"].append(timed(ode, lambda: ode.residual(dt, dt, y, lhs, f), reps, 10))
            row["jacobian_us"].append(timed(ode, lambda: ode.jacobian(dt, dt, y, lhs), jac_reps, 2))
            p0, w0 = ode.network_stats()
            ode.residual(dt, dt, y, lhs, f)
            p1, w1 = ode.network_stats()
            ode.jacobian(dt, dt, y, lhs)
            p2, w2 = ode.network_stats()
            row["residual_passes_waits"] = (p1 - p0, w1 - w0)
            row["jacobian_passes_waits"] = (p2 - p1, w2 - w1)
    ode.set_network_pass("host")
    res = {"coupling_cells": int(len(ode.network_couplings()[0]))}
    for m in MODES:
        for key in ("residual_us", "jacobian_us"):
            v = np.array(out[m][key])
            out[m][key[:-3] + "_spread"] = float((v.max() - v.min()) / np.median(v))
            out[m][key] = float(np.median(v))
        res[m] = out[m]
    res["residual_host_over_device"] = res["host"]["residual_us"] / res["device"]["residual_us"]
    res["jacobian_host_over_device"] = res["host"]["jacobian_us"] / res["device"]["jacobian_us"]
    return res


def reinjection(a):
    from waiwera_amd.simulation import Simulation
    inp = json.load(open(os.path.join(INPUTS, "reinjection.json")))
    sim = Simulation(inp, base_dir=INPUTS, mesh_file=os.path.join(INPUTS, "greinjection.dat"))
    sim.ts.run(num_steps=3)          # wells flowing, limiter / reinjector at work
    y = np.asarray(sim.y, dtype=np.float64).copy()
    row = dict(case="reinjection benchmark", cells=int(sim.ode.n_owned), sources=len(inp.get("source", [])))
    row.update(measure(sim.ode, y, 1.0e5, a.rounds, a.reps, a.jac_reps))
    sim.ode.destroy()
    return row


def synthetic(wells, a):
    """32 x 32 x 8, `wells` networked wells in cells of their own: three quarters produce, one quarter is fed"""
    from waiwera_amd import lib as wl
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(32, 32, 8), brick=(16, 16, 2), eos="we", lens=True, sources=False)
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    cells = np.linspace(0, lm.n_owned - 1, wells).astype(np.int32)
    n_prod = (3 * wells) // 4
    prod, inj = list(range(n_prod)), list(range(n_prod, wells))
    rate = np.where(np.arange(wells) < n_prod, -5.0, 2.0)
    enth = np.where(np.arange(wells) < n_prod, 0.0, 4.0e5)
    P = lambda v: v.ctypes.data_as(wl.pi if v.dtype == np.int32 else wl.pd)   # noqa: E731
    c, r, e, k = wl._i32(cells), wl._f64(rate), wl._f64(enth), wl._i32(np.where(np.arange(wells) < n_prod, 0, 1))
    sim._chk(wl.LIB.wai_set_sources(sim.h, wells, P(c), P(r), P(e), P(k)), "set_sources")
    recs = [dict(kind="deliverability", coef=1.0e-11, pressure=2.0e5) if i < n_prod else dict() for i in range(wells)]
    sim._chk(wl.LIB.wai_set_source_controls(sim.h, wl.source_controls(recs)), "set_source_controls")
    half = n_prod // 2
    sep = [(640.0e3, 2748.0e3)]
    spec = dict(rate_specified=[1] * wells, enthalpy_specified=[int(i >= n_prod) for i in range(wells)],
                groups=[dict(inputs=[(1, i) for i in prod[:half]], scaling=0, limits=[(0, 1.5 * half)], separator=sep),
                        dict(inputs=[(1, i) for i in prod[half:]], scaling=1, limits=[(0, 1.5 * (n_prod - half))], separator=sep),
                        dict(inputs=[(2, 0), (2, 1)], scaling=0, limits=[], separator=None)],
                reinjectors=[dict(input=(2, 2), overflow=(1, inj[-1]),
                                  outputs=[dict(flow=1, out=(1, i), rate=-1.0, proportion=0.8 / max(len(inj) - 1, 1), enthalpy=-1.0)
                                           for i in inj[:-1]])])
    sim.set_source_network(spec)
    y = scaled(prim, region, "we").ravel().copy()
    row = dict(case="synthetic 32 x 32 x 8", cells=int(lm.n_owned), sources=wells)
    row.update(measure(sim, y, 2.0e4, a.rounds, a.reps, max(1, a.jac_reps // max(1, wells // 8))))
    sim.destroy()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=300, help="wai_residual calls per timing")
    ap.add_argument("--jac-reps", type=int, default=16, help="wai_jacobian calls per timing (fewer for more wells)")
    ap.add_argument("--wells", type=int, nargs="*", default=[8, 64, 256])
    ap.add_argument("--no-reinjection", action="store_true")
    a = ap.parse_args()
    if not a.no_reinjection:
        print(json.dumps(reinjection(a)), flush=True)
    for w in a.wells:
        print(json.dumps(synthetic(w, a)), flush=True)


if __name__ == "__main__":
    main()
