"""Times block-Jacobi ILU(0) in its two elimination orders (wai_set_pc_ordering) in ONE process, alternating: natural (the
default: k_pc_park on 16 x 16 x 2 bricks, k_lvl_solve per level under one block per rank) against multicolour (k_pc_colour on
the bricks, k_colour_sweep per colour under one block per rank).  Per case and ordering, on the Jacobian and residual of
the bench case's initial state (eos we, two-phase lens):

- apply_ms: one preconditioner application z = B^-1 r (wai_pc_apply on device vectors inside the device-event timer), two
  warm-ups then the median of 7, per round; the natural order is also timed against itself (A/A) and the spread of those
  repeats is the bar a difference has to clear;
- ksp_its, ksp_ms_per_it: one BiCGStab solve of that system at the default rtol 1e-5 inside the device-event timer -- an
  iteration is two preconditioned-operator applications and the vector updates, so iterations x time can be read off;
- steps: Newton and Krylov iteration counts of the first accepted time steps from dt = 1e4 s, doubling (--steps).

One JSON line per case:

    python tools/pc_colour_timing.py > profiles/pc_colour_timing.json     # 100^3 and 216^3 (216^3 needs minutes of set-up)
    python tools/pc_colour_timing.py --small                              # 48 x 48 x 16 and 100^3
    python tools/pc_colour_timing.py --dims 216 216 216 --no-one-block    # one size, one kind of subdomain"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.pc_tiles_timing import DeviceVector, launches, median_ms  # noqa: E402
from waiwera_amd.cases import make_case, scaled  # noqa: E402
from waiwera_amd.flow_simulation import FlowSimulation  # noqa: E402

BRICK = (16, 16, 2)
ORDERS = ("natural", "multicolour")


def system(dims, one_block):
    g, lm, prim, region = make_case(dims=dims, brick=BRICK, eos="we", lens=True)
    if one_block:
        lm.sub_ptr = None
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    y = scaled(prim, region, "we").ravel().copy()
    return sim, y


def first_system(sim, y, dt=1.0e4):
    """the Jacobian of the initial state in force, and its residual"""
    n = sim.num_dof
    L, f = np.zeros(n), np.zeros(n)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, 1.0, y, L)
    assert sim.residual(0.0, dt, y, L, f) == 0
    assert sim.jacobian(0.0, dt, y, L) == 0
    return f


def measure(sim, f, rounds):
    n = sim.num_dof
    r = DeviceVector(np.random.default_rng(1).normal(size=n))
    z = DeviceVector(np.zeros(n))
    out = {o: dict(apply_ms=[], ksp_its=[], ksp_ms_per_it=[]) for o in ORDERS}
    again = []
    for _ in range(rounds):
        for o in ORDERS:
            sim.set_pc_ordering(o)
            assert sim.pc_setup() == 0
            row = out[o]
            row["kernel"] = sim.pc_kernel_name()
            row["apply_launches"] = launches(sim, r, z)
            row["apply_ms"].append(median_ms(sim, r, z))
            if o == "natural":
                again.append(median_ms(sim, r, z))
            x = np.zeros(n)
            sim.ksp_solve(f, x)                     # warm-up
            x[:] = 0.0
            sim.timer_start()
            its, reason, rn = sim.ksp_solve(f, x)
            ms = sim.timer_stop()
            assert reason > 0, (o, reason)
            row["ksp_its"].append(its)
            row["ksp_ms_per_it"].append(ms / max(its, 1))
    out["multicolour"]["max_colours"] = sim.pc_ordering()[1]
    nat = np.array(out["natural"]["apply_ms"] + again)
    out["natural_spread"] = float((nat.max() - nat.min()) / np.median(nat))      # A/A
    out["apply_ratio_natural_over_multicolour"] = float(np.median(nat) / np.median(out["multicolour"]["apply_ms"]))
    a = np.median(out["natural"]["ksp_ms_per_it"]) * np.median(out["natural"]["ksp_its"])
    b = np.median(out["multicolour"]["ksp_ms_per_it"]) * np.median(out["multicolour"]["ksp_its"])
    out["solve_ratio_natural_over_multicolour"] = float(a / b)
    sim.set_pc_ordering("natural")
    r.free(); z.free()
    return out


def steps(dims, one_block, nsteps):
    """Newton and Krylov counts of the first accepted time steps, per ordering (a fresh context each)"""
    out = {}
    for o in ORDERS:
        sim, y = system(dims, one_block)
        sim.set_pc_ordering(o)
        t, dt, rows = 0.0, 1.0e4, []
        while len(rows) < nsteps and dt > 1.0:
            y0 = y.copy()
            sim.timer_start()
            reason, nits, kits = sim.timestep(t, dt, y)
            ms = sim.timer_stop()
            if reason > 0:
                rows.append(dict(dt=dt, newton=nits, krylov=kits, step_ms=ms))
                t += dt
                dt *= 2.0
            else:
                y[:] = y0
                dt *= 0.2
        out[o] = rows
        sim.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="48 x 48 x 16 and 100^3 instead of 100^3 and 216^3")
    ap.add_argument("--dims", type=int, nargs=3, default=None, help="this one size only")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="accepted time steps counted per ordering (0: none)")
    ap.add_argument("--no-one-block", action="store_true", help="without the one-block-per-rank cases")
    ap.add_argument("--no-bricks", action="store_true", help="without the brick cases")
    a = ap.parse_args()
    sizes = [(48, 48, 16), (100, 100, 100)] if a.small else [(100, 100, 100), (216, 216, 216)]
    if a.dims:
        sizes = [tuple(a.dims)]
    for dims in sizes:
        for one_block in (False, True):
            if (one_block and a.no_one_block) or (not one_block and a.no_bricks):
                continue
            sim, y = system(dims, one_block)
            f = first_system(sim, y)
            row = dict(case="one block per rank" if one_block else "bricks 16 x 16 x 2", dims=dims, n=sim.num_dof // 2)
            row.update(measure(sim, f, a.rounds))
            sim.destroy()
            if a.steps > 0:
                row["steps"] = steps(dims, one_block, a.steps)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
