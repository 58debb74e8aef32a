"""Times the two-level preconditioner (wai_set_pc_coarse) against one level in ONE process, the variants alternating, on the
first linear system of the bench cases (eos we, two-phase lens, 16 x 16 x 2 bricks, block Jacobi ILU(0), BiCGStab at the
default rtol 1e-5): the Jacobian and residual of the initial state at dt = 1e4 s.  Variants:

- one_level            the default path (the fused launches; what the parent of this change runs)
- one_level_unfused    one level on the route a coarse level puts the system on (WAI_PC_UNFUSED=1: k_spmv, the fused kernel
                       as a solve, separate reductions)
- additive_N, deflated_N   the coarse level over N = 64, 216, 512 aggregates (4^3, 6^3, 8^3 boxes)

Per variant and round: Krylov iterations, ms per iteration, ms per solve (device-event timer around wai_ksp_solve after a
warm-up solve), kernel launches per iteration, and the set-up's ms -- whole (wai_pc_setup inside the timer) and, for the
coarse level, the Galerkin product and the inversion apart (the library's own events, profiling on for the set-up only).
A variant's own repeats give its spread; a difference inside the spreads is no difference.  One JSON line per case:

    python tools/pc_coarse_timing.py > profiles/pc_coarse_timing.json     # 100^3 and 216^3
    python tools/pc_coarse_timing.py --small                              # 48 x 48 x 16 only"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.pc_colour_timing import first_system, system  # noqa: E402

BOXES = {64: (4, 4, 4), 216: (6, 6, 6), 512: (8, 8, 8)}


def variants(counts):
    v = [("one_level", None, None), ("one_level_unfused", None, None)]
    for mode in ("additive", "deflated"):
        v += [("%s_%d" % (mode, n), mode, n) for n in counts]
    return v


def measure(sim, f, rounds, counts):
    n = sim.num_dof
    out = {name: dict(ksp_its=[], ms_per_it=[], ms_per_solve=[], setup_ms=[], galerkin_ms=[], inverse_ms=[], launches_per_it=[])
           for name, _, _ in variants(counts)}
    for _ in range(rounds):
        for name, mode, nagg in variants(counts):
            os.environ.pop("WAI_PC_UNFUSED", None)
            if name == "one_level_unfused":
                os.environ["WAI_PC_UNFUSED"] = "1"
            if mode is None:
                sim.set_pc_coarse("off")
            else:
                sim.set_pc_coarse(mode, boxes=BOXES[nagg])
            row = out[name]
            sim.set_sub_pc("lu")       # a setting changed and changed back: the next set-up is a full one on the same values
            sim.set_sub_pc("ilu")
            sim.profile(True)
            sim.timer_start()
            assert sim.pc_setup() == 0
            row["setup_ms"].append(sim.timer_stop())
            sim.profile(False)
            if mode is not None:
                t = np.zeros(2)
                sim.test_coarse("times", None, t)
                row["galerkin_ms"].append(float(t[0]))
                row["inverse_ms"].append(float(t[1]))
            row["kernel"] = sim.pc_kernel_name()
            x = np.zeros(n)
            sim.ksp_solve(f, x)                     # warm-up
            x[:] = 0.0
            k0 = sim.launch_stats()[0]
            sim.timer_start()
            its, reason, rn = sim.ksp_solve(f, x)
            ms = sim.timer_stop()
            assert reason > 0, (name, reason)
            row["ksp_its"].append(its)
            row["ms_per_it"].append(ms / max(its, 1))
            row["ms_per_solve"].append(ms)
            row["launches_per_it"].append((sim.launch_stats()[0] - k0) / max(its, 1))
    os.environ.pop("WAI_PC_UNFUSED", None)
    sim.set_pc_coarse("off")
    base = np.array(out["one_level"]["ms_per_solve"])
    out["one_level_spread"] = float((base.max() - base.min()) / np.median(base))
    for name in out:
        if isinstance(out[name], dict) and name != "one_level":
            out[name]["solve_ratio_over_one_level"] = float(np.median(out[name]["ms_per_solve"]) / np.median(base))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="48 x 48 x 16 instead of 100^3 and 216^3")
    ap.add_argument("--dims", type=int, nargs=3, default=None, help="this one size only")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--aggregates", type=int, nargs="+", default=[64, 216, 512], choices=sorted(BOXES))
    a = ap.parse_args()
    sizes = [(48, 48, 16)] if a.small else [(100, 100, 100), (216, 216, 216)]
    if a.dims:
        sizes = [tuple(a.dims)]
    for dims in sizes:
        sim, y = system(dims, False)
        f = first_system(sim, y)
        row = dict(case="bricks 16 x 16 x 2, bjacobi ILU(0), bcgs", dims=dims, n=sim.num_dof // 2)
        row.update(measure(sim, f, a.rounds, a.aggregates))
        sim.destroy()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
