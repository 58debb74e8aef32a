"""Measures what the compact cell order (Simulation(cell_order="compact"), wai_cell_order) does to the linear solves of an
input-file run, in ONE process, the orders alternating.  The workload: a layered hexahedral mesh of 100 x 100 x 20 m cells
(thin layers: a vertical transmissibility is 25 x a horizontal one; two rock types, a source pair, open top), eos we,
written as a gmsh 2.2 ASCII file x-fastest / z-slowest and again with its elements scrambled (seeded).  Default size
64 x 48 x 20 = 61 440 cells: about what unstructured.build_mesh makes in a minute.  Four variants -- file and scrambled,
each under cell_order "input" and "compact" at the default cap of 512 rows -- under the preconditioners bjacobi and asm.

Per variant and preconditioner:
- steps: the same fixed sequence of time steps from the initial state (--dts), Newton and Krylov iterations of each and
  krylov_per_newton over the sequence.  A step that fails is recorded as failed, and the sequence goes on from the state
  before it: no variant gets another sequence;
- ksp_its, ksp_ms, ksp_ms_per_it: one BiCGStab solve of the first step's first Newton system at the default rtol 1e-5 inside
  the device-event timer, after a warm-up solve, the median over --rounds (the variants alternate inside a round); the
  "input" variants are timed twice per round, and the spread of all those repeats is the bar a difference has to clear;
- kernel: pc_kernel_name(); cut_before / cut_after: the share of interior faces the subdomains cut.

One JSON document:

    python tools/cell_order_timing.py > profiles/cell_order_timing.json
    python tools/cell_order_timing.py --dims 16 12 10 --rows 256          # a rehearsal size"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waiwera_amd.simulation import Simulation  # noqa: E402

SPACING = (100.0, 100.0, 20.0)
PCS = ("bjacobi", "asm")


def write_msh(path, dims, order):
    """the hex grid as gmsh 2.2 ASCII; element k of the file is cell order[k] of the x-fastest numbering"""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    xyz = np.stack([i.ravel() * SPACING[0], j.ravel() * SPACING[1], k.ravel() * SPACING[2]], axis=1)
    node = lambda i_, j_, k_: (k_ * (ny + 1) + j_) * (nx + 1) + i_ + 1      # noqa: E731
    c = np.asarray(order)
    i0, j0, k0 = c % nx, (c // nx) % ny, c // (nx * ny)
    el = np.stack([node(i0, j0, k0), node(i0 + 1, j0, k0), node(i0 + 1, j0 + 1, k0), node(i0, j0 + 1, k0),
                   node(i0, j0, k0 + 1), node(i0 + 1, j0, k0 + 1), node(i0 + 1, j0 + 1, k0 + 1), node(i0, j0 + 1, k0 + 1)], axis=1)
    with open(path, "w") as f:
        f.write("$MeshFormat\n2.2 0 8\n$EndMeshFormat\n$Nodes\n%d\n" % len(xyz))
        f.writelines("%d %.17g %.17g %.17g\n" % (q + 1, p[0], p[1], p[2]) for q, p in enumerate(xyz))
        f.write("$EndNodes\n$Elements\n%d\n" % len(el))
        f.writelines("%d 5 2 1 1 %s\n" % (q + 1, " ".join(map(str, e))) for q, e in enumerate(el.tolist()))
        f.write("$EndElements\n")


def make_input(dims, filename, number):
    """number[c]: the file's number of x-fastest cell c"""
    nx, ny, nz = dims
    n = nx * ny * nz
    where = np.empty(n, dtype=np.int64)
    where[number] = np.arange(n)
    k = np.arange(n) // (nx * ny)
    depth = (nz - 0.5 - k) * SPACING[2]
    primary = np.stack([1.0e5 + 9.0e3 * depth, 20.0 + 0.25 * depth], axis=1)
    cell = lambda cells: [int(number[c]) for c in np.atleast_1d(cells)]      # noqa: E731
    return {
        "mesh": {"filename": filename}, "eos": {"name": "we"}, "gravity": 9.8,
        "rock": {"types": [{"name": "base", "permeability": [1.0e-13, 1.0e-13, 2.0e-14], "porosity": 0.1, "zones": "all"},
                           {"name": "tight", "permeability": [2.0e-14, 2.0e-14, 5.0e-15], "porosity": 0.08,
                            "cells": cell(np.arange(0, nx * ny * max(nz // 5, 1)))}]},
        "initial": {"primary": primary[where].tolist(), "region": [1] * n},
        "boundaries": [{"primary": [1.0e5, 20.0], "region": 1, "faces": {"cells": cell(np.arange(n - nx * ny, n)), "normal": [0, 0, 1]}}],
        "source": [{"cell": cell(nx // 3 + nx * (ny // 2) + nx * ny)[0], "rate": 2.0, "enthalpy": 4.0e5},
                   {"cell": cell(n - 1 - nx * ny * 2 - nx)[0], "rate": -1.0}],
        "time": {"start": 0.0, "stop": 1.0e9, "step": {"size": 1.0e5, "solver": {"nonlinear": {"maximum": {"iterations": 12}}}}},
        "output": False,
    }


def first_system(ode, y, dt):
    n = ode.num_dof
    L, f = np.zeros(n), np.zeros(n)
    assert ode.pre_eval(0.0, y) == 0
    ode.lhs(0.0, 1.0, y, L)
    assert ode.residual(0.0, dt, y, L, f) == 0
    assert ode.jacobian(0.0, dt, y, L) == 0
    return f


def timed_solve(ode, f):
    x = np.zeros(ode.num_dof)
    ode.ksp_solve(f, x)                     # warm-up
    x[:] = 0.0
    ode.timer_start()
    its, reason, rn = ode.ksp_solve(f, x)
    ms = ode.timer_stop()
    return its, reason, ms


def run_steps(ode, y0, dts):
    y, t, rows = y0.copy(), 0.0, []
    for dt in dts:
        keep = y.copy()
        ode.timer_start()
        reason, nits, kits = ode.timestep(t, dt, y)
        ms = ode.timer_stop()
        rows.append(dict(dt=dt, converged=bool(reason > 0), newton=nits, krylov=kits, step_ms=ms))
        if reason > 0:
            t += dt
        else:
            y[:] = keep
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(64, 48, 20))
    ap.add_argument("--rows", type=int, default=None, help="subdomain_rows (default: the front end's 512)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dts", type=float, nargs="+", default=(1.0e5, 2.0e5, 4.0e5, 8.0e5))
    a = ap.parse_args()
    dims = tuple(a.dims)
    n = int(np.prod(dims))
    doc = dict(workload="layered hex mesh %d x %d x %d of 100 x 100 x 20 m cells, eos we, gravity on" % dims, n=n,
               subdomain_rows=a.rows or 512, dts=list(a.dts), rounds=a.rounds, variants={})
    with tempfile.TemporaryDirectory() as d:
        p = np.random.default_rng(7).permutation(n)
        number = np.empty(n, dtype=np.int64)
        number[p] = np.arange(n)
        files = {"file": (np.arange(n), np.arange(n)), "scrambled": (p, number)}
        sims = {}
        for name, (order, num) in files.items():
            write_msh(os.path.join(d, name + ".msh"), dims, order)
            for co in ("input", "compact"):
                t0 = time.time()
                s = Simulation(make_input(dims, name + ".msh", num), base_dir=d, default_pc="bjacobi", cell_order=co, subdomain_rows=a.rows)
                sims[(name, co)] = s
                ch = s.cell_order_choice
                doc["variants"]["%s/%s" % (name, co)] = dict(setup_s=time.time() - t0, n_sub=ch.n_sub, largest_subdomain=ch.largest_subdomain,
                                                             cut_before=ch.cut_before, cut_after=ch.cut_after)
                print("set up %s/%s in %.1f s" % (name, co, time.time() - t0), file=sys.stderr, flush=True)
        for pc in PCS:
            acc = {k: dict(ksp_its=[], ksp_ms=[], again_ms=[]) for k in sims}
            fs = {}
            for k, s in sims.items():
                s.ode.set_opts(pc_type=pc)
                fs[k] = first_system(s.ode, s.y, a.dts[0])
            for _ in range(a.rounds):
                for k, s in sims.items():           # the variants alternate inside a round
                    its, reason, ms = timed_solve(s.ode, fs[k])
                    assert reason > 0, (k, pc, reason)
                    acc[k]["ksp_its"].append(its)
                    acc[k]["ksp_ms"].append(ms)
                    if k[1] == "input":             # A/A
                        acc[k]["again_ms"].append(timed_solve(s.ode, fs[k])[2])
            for k, s in sims.items():
                its, ms = float(np.median(acc[k]["ksp_its"])), float(np.median(acc[k]["ksp_ms"]))
                row = dict(kernel=s.ode.pc_kernel_name(), ksp_its=its, ksp_ms=ms, ksp_ms_per_it=ms / max(its, 1.0), ksp_ms_all=acc[k]["ksp_ms"])
                if acc[k]["again_ms"]:
                    both = np.array(acc[k]["ksp_ms"] + acc[k]["again_ms"])
                    row["spread"] = float((both.max() - both.min()) / np.median(both))
                steps = run_steps(s.ode, s.y, a.dts)
                nn, kk = sum(r["newton"] for r in steps), sum(r["krylov"] for r in steps)
                row.update(steps=steps, krylov_per_newton=kk / max(nn, 1), ms_per_linear_solve_first_system=ms)
                doc["variants"]["%s/%s" % k][pc] = row
                print("%s %s/%s: %s" % (pc, k[0], k[1], {q: row[q] for q in ("kernel", "ksp_its", "ksp_ms", "krylov_per_newton")}), file=sys.stderr, flush=True)
        for s in sims.values():
            s.ode.destroy()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
