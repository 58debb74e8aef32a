"""Times wai_jacobian with the three ways of building the source network's coupling blocks -- the column loop with the host
pass ("host"), the column loop with the device pass ("columns") and the batched build (wai_set_coupling_build, "batched") -- in
ONE process, the modes alternating: a host clock around `reps` calls that end in a device synchronise, warm-ups first,
`rounds` rounds per mode; the median over the rounds and their spread ((max - min) / median) per mode -- the bar a difference
between the modes has to clear.  Launches, columns and chunks of a build, its passes and its stream waits come from the
library's own counters (wai_test_coupling_build_stats, wai_test_network_stats).  The blocks of the three modes are compared
bit for bit on the way.

Cases: those of tools/network_device_timing.py -- the reference's reinjection benchmark after three time steps, and its
synthetic 32 x 32 x 8 mesh with 8, 64 and 256 networked wells.  One JSON line per case:

    python tools/coupling_build_timing.py > profiles/coupling_build_timing.json
    python tools/coupling_build_timing.py --wells 8 --no-reinjection          # one synthetic size, quickly"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import network_device_timing as ndt  # noqa: E402

MODES = (("host", "host", "columns"), ("columns", "device", "columns"), ("batched", "device", "batched"))


def measure(ode, y, dt, rounds, jac_reps):
    n = ode.n_owned * ode.num_primary_variables
    f, lhs = np.zeros(n), np.zeros(n)
    assert ode.pre_eval(0.0, y) == 0
    ode.lhs(0.0, (0.0, 0.0), y, lhs)
    out = {m: dict(jacobian_us=[]) for m, _, _ in MODES}
    blocks = {}
    for _ in range(rounds):
        for m, where, how in MODES:
            ode.set_network_pass(where)
            ode.set_coupling_build(how)
            assert ode.network_pass() == (where, where) and ode.coupling_build() == (how, how), (ode.network_pass(), ode.coupling_build())
            row = out[m]
            ode.residual(dt, dt, y, lhs, f)
            row["jacobian_us"].append(ndt.timed(ode, lambda: ode.jacobian(dt, dt, y, lhs), jac_reps, 2))
            p0, w0 = ode.network_stats()
            ode.jacobian(dt, dt, y, lhs)
            p1, w1 = ode.network_stats()
            row["passes_waits"] = (p1 - p0, w1 - w0)
            row["launches_columns_chunks"] = ode.coupling_build_stats()
            blocks[m] = ode.network_couplings()[1]
    ode.set_network_pass("host")
    ode.set_coupling_build("columns")
    res = {"coupling_cells": int(len(ode.network_couplings()[0]))}
    for m, _, _ in MODES:
        v = np.array(out[m]["jacobian_us"])
        out[m]["jacobian_spread"] = float((v.max() - v.min()) / np.median(v))
        out[m]["jacobian_us"] = float(np.median(v))
        res[m] = out[m]
        res[m]["same_bits_as_host"] = bool(np.array_equal(blocks[m].view(np.uint64), blocks["host"].view(np.uint64)))
    best = min(("host", "columns"), key=lambda m: res[m]["jacobian_us"])
    ratio = res[best]["jacobian_us"] / res["batched"]["jacobian_us"]
    spread = max(res[best]["jacobian_spread"], res["batched"]["jacobian_spread"])
    res["faster_existing_mode"] = best
    res["existing_over_batched"] = ratio
    # a gain or a loss only where the difference exceeds the recorded repeat spread of the two modes compared
    res["verdict"] = "FASTER" if ratio > 1.0 + spread else ("SLOWER" if ratio < 1.0 / (1.0 + spread) else "WITHIN SPREAD")
    return res


def reinjection(a):
    from waiwera_amd.simulation import Simulation
    inp = json.load(open(os.path.join(ndt.INPUTS, "reinjection.json")))
    sim = Simulation(inp, base_dir=ndt.INPUTS, mesh_file=os.path.join(ndt.INPUTS, "greinjection.dat"))
    sim.ts.run(num_steps=3)          # wells flowing, limiter / reinjector at work
    y = np.asarray(sim.y, dtype=np.float64).copy()
    row = dict(case="reinjection benchmark", cells=int(sim.ode.n_owned), sources=len(inp.get("source", [])))
    row.update(measure(sim.ode, y, 1.0e5, a.rounds, a.jac_reps))
    sim.ode.destroy()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--jac-reps", type=int, default=16, help="wai_jacobian calls per timing (fewer for more wells)")
    ap.add_argument("--wells", type=int, nargs="*", default=[8, 64, 256])
    ap.add_argument("--no-reinjection", action="store_true")
    a = ap.parse_args()
    a.reps = 0
    if not a.no_reinjection:
        print(json.dumps(reinjection(a)), flush=True)
    # that tool's synthetic case -- it builds the mesh, the wells and the network, then calls its module's measure -- measured
    # this tool's way
    ndt.measure = lambda ode, y, dt, rounds, reps, jac_reps: measure(ode, y, dt, rounds, jac_reps)
    for w in a.wells:
        print(json.dumps(ndt.synthetic(w, a)), flush=True)


if __name__ == "__main__":
    main()
