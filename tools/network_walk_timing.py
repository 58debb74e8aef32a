"""Times wai_residual and wai_jacobian with the source network's pass on the host, on the device with the lane walk and on
the device with the wave walk (wai_set_network_walk), the Jacobian under both coupling builds (wai_set_coupling_build), in
ONE process with the modes alternating -- the cases and the method of tools/network_device_timing.py: a host clock around
`reps` calls that end in a device synchronise, warm-ups first, `rounds` rounds per mode; the median over the rounds and their
spread ((max - min) / median) per mode, the bar a difference between two modes has to clear.  Passes and stream waits per
call come from the library's counters (wai_test_network_stats), launches of a coupling build from
wai_test_coupling_build_stats.  A mode that is not in force for a case (the lane walk for a network above 64 KB of LDS) is
recorded as such with what ran in its place, and not timed.

Cases: the reference's reinjection benchmark after three time steps, and synthetic 32 x 32 x 8 meshes with 8, 64, 256 and 512
networked wells (512: a size only the wave walk holds on the device).  One JSON line per case:

    python tools/network_walk_timing.py > profiles/network_walk_timing.json
    python tools/network_walk_timing.py --wells 8 --reps 20 --no-reinjection          # one synthetic size, quickly"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import network_device_timing as base  # noqa: E402

MODES = (("host", "host", "lane"), ("lane", "device", "lane"), ("wave", "device", "wave"))
BUILDS = ("columns", "batched")


def measure(ode, y, dt, rounds, reps, jac_reps):
    from waiwera_amd import lib as wl
    n = ode.n_owned * ode.num_primary_variables
    f, lhs = np.zeros(n), np.zeros(n)
    assert ode.pre_eval(0.0, y) == 0
    ode.lhs(0.0, (0.0, 0.0), y, lhs)
    out = {}
    for name, where, walk in MODES:
        ode.set_network_pass(where)
        ode.set_network_walk(walk)
        limit, needed = C.c_int(0), C.c_int(0)
        ode._chk(wl.LIB.wai_test_network_lds(ode.h, C.byref(limit), C.byref(needed)), "network_lds")
        out[name] = dict(in_force=dict(network_pass=ode.network_pass()[1], network_walk=ode.network_walk()[1]),
                         lds_doubles=needed.value, lds_limit=limit.value, residual_us=[])
        out[name]["timed"] = out[name]["in_force"] == dict(network_pass=where, network_walk=walk)
        for b in BUILDS:
            out[name]["jacobian_%s_us" % b] = []
    for _ in range(rounds):
        for name, where, walk in MODES:
            row = out[name]
            if not row["timed"]:
                continue
            ode.set_network_pass(where)
            ode.set_network_walk(walk)
            row["residual_us"].append(base.timed(ode, lambda: ode.residual(dt, dt, y, lhs, f), reps, 10))
            p0, w0 = ode.network_stats()
            ode.residual(dt, dt, y, lhs, f)
            p1, w1 = ode.network_stats()
            row["residual_passes_waits"] = (p1 - p0, w1 - w0)
            for b in BUILDS:
                ode.set_coupling_build(b)
                if ode.coupling_build()[1] != b:      # (the host pass has the column loop alone)
                    continue
                row["jacobian_%s_us" % b].append(base.timed(ode, lambda: ode.jacobian(dt, dt, y, lhs), jac_reps, 2))
                p1, w1 = ode.network_stats()
                ode.jacobian(dt, dt, y, lhs)
                p2, w2 = ode.network_stats()
                row["jacobian_%s_passes_waits" % b] = (p2 - p1, w2 - w1)
                row["jacobian_%s_launches" % b] = ode.coupling_build_stats()[0]
            ode.set_coupling_build("columns")
    ode.set_network_pass("host")
    ode.set_network_walk("lane")
    res = {"coupling_cells": int(len(ode.network_couplings()[0]))}
    for name, _, _ in MODES:
        row = out[name]
        for key in ["residual_us"] + ["jacobian_%s_us" % b for b in BUILDS]:
            v = np.array(row.pop(key))
            if v.size:
                row[key], row[key[:-3] + "_spread"] = float(np.median(v)), float((v.max() - v.min()) / np.median(v))
        res[name] = row
    for key in ["residual_us"] + ["jacobian_%s_us" % b for b in BUILDS]:
        for other in ("lane", "host"):
            if key in res["wave"] and key in res[other]:
                res["%s_%s_over_wave" % (key[:-3], other)] = res[other][key] / res["wave"][key]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=300, help="wai_residual calls per timing")
    ap.add_argument("--jac-reps", type=int, default=16, help="wai_jacobian calls per timing (fewer for more wells)")
    ap.add_argument("--wells", type=int, nargs="*", default=[8, 64, 256, 512])
    ap.add_argument("--no-reinjection", action="store_true")
    a = ap.parse_args()
    base.measure = measure      # the cases of tools/network_device_timing.py, measured in this tool's modes
    if not a.no_reinjection:
        print(json.dumps(base.reinjection(a)), flush=True)
    for w in a.wells:
        print(json.dumps(base.synthetic(w, a)), flush=True)


if __name__ == "__main__":
    main()
