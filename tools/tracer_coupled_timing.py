#!/usr/bin/env python
"""Timing of one auxiliary (tracer) solve at C2 size -- 100^3 eos we, 16 x 16 x 2 bricks -- after a converged flow step,
for nt = 1, 2, 4, 8 tracers:

    python tools/tracer_coupled_timing.py [--parent-tree DIR] [--nt 1 2 4 8] [--out profiles/tracer_coupled_timing.json]

  (a) parent      wai_tracer_solve of the commit before the coupled mode: a built checkout of it under DIR (optional; the
                  worker below runs with DIR as its package root, in a process of its own),
  (b) per_tracer  this tree, WAI_TRACER_PER_TRACER -- the same code as (a): the two must agree within the box spread,
  (c) coupled     this tree, WAI_TRACER_COUPLED.

Each variant is a fresh process (its own context and library).  GMRES(30), rtol 1e-5 (the auxiliary defaults), backward
Euler, block-Jacobi ILU(0).  A solve is timed with the library's HIP-event timer around wai_tracer_solve (device arrays in
and out), after two warm-up solves, the median of `--reps`; launches and scalar reads from wai_launch_stats.  The fused
operator of the coupled mode is timed by the per-class profile (class pc_apply: k_dg_pc's applications, one of them the
plain B^-1 b of the solve's start) in one more solve, and set against the byte model of DESIGN.md section 4:
n_owned * (7 (8 nt + 4) + 7 * 8 nt + 16 nt) bytes per application, as a share of the 8 TB/s HBM peak."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12
PHASES = [0, 1, 0, 1, 1, 0, 0, 1]
DECAY = [1e-8, 1e-7, 2e-7, 3e-8, 5e-8, 4e-7, 6e-8, 9e-8]
DIFF = [1e-6, 2e-5, 0.0, 3e-6, 1e-5, 0.0, 2e-6, 4e-6]


def worker(mode, nts, reps):
    """runs inside the tree named by sys.path[0]; prints one JSON line"""
    import numpy as np
    import torch
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(100, 100, 100), brick=(16, 16, 2), eos="we", lens=True)
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    y = scaled(prim, region).ravel().copy()
    dt = 2.0e3
    reason, nits, kits = sim.timestep(0.0, dt, y)
    assert reason > 0, reason
    rows = []
    dev = torch.device("cuda")
    for nt in nts:
        rng = np.random.default_rng(11)
        bc = rng.uniform(0, 1e-3, (lm.n_bc, nt))
        inj = np.where(np.asarray(lm.src_rate)[:, None] > 0, rng.uniform(0, 1e-2, (lm.n_src, nt)), 0.0)
        sim.set_tracers(PHASES[:nt], DECAY[:nt], [0.0] * nt, DIFF[:nt], bc=bc, injection=inj)
        sim.set_aux_solver("gmres")
        if mode != "parent":
            sim.set_tracer_solve_mode(mode)
        n = lm.n_owned * nt
        Al = np.zeros(n)
        sim.aux_lhs(0.0, None, Al)
        alx = torch.from_numpy(Al * rng.uniform(0, 1e-3, n)).to(dev)
        X, new = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
        for _ in range(2):
            r, its = sim.aux_solve("beuler", dt, 1.0, alx, None, X, new)
        assert r > 0, (nt, r)
        ms = []
        k0, c0 = sim.launch_stats()
        for _ in range(reps):
            sim.timer_start()
            r, its = sim.aux_solve("beuler", dt, 1.0, alx, None, X, new)
            ms.append(sim.timer_stop())
        k1, c1 = sim.launch_stats()
        row = dict(nt=nt, ms_per_solve=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), iterations=int(its),
                   reason=int(r), launches=(k1 - k0) // reps, scalar_reads=(c1 - c0) // reps,
                   ms_per_iteration=float(np.median(ms)) / max(int(its), 1))
        if mode == "coupled" and nt > 1:
            sim.profile(True)
            sim.aux_solve("beuler", dt, 1.0, alx, None, X, new)
            prof = sim.profile_get()
            pms, pn = prof["pc_apply"]
            sim.profile(False)
            # where the rest of a solve goes: the ILU(0) pass (class pc_setup) and the Krylov vector kernels; the assembly
            # sweep belongs to no class (solve - the classes, roughly: the profiled solve runs without speculation)
            row.update(ilu_setup_ms=prof["pc_setup"][0], vector_ms=prof["vector"][0], spmv_ms=prof["spmv"][0])
            nbytes = lm.n_owned * (7 * (8 * nt + 4) + 7 * 8 * nt + 16 * nt)
            row.update(operator_ms=pms / max(pn, 1), operator_applications=int(pn), operator_bytes=int(nbytes),
                       operator_share_of_hbm_peak=nbytes / (pms / max(pn, 1) * 1e-3) / PEAK)
        rows.append(row)
    sim.destroy()
    print("RESULT " + json.dumps(dict(mode=mode, cells=int(lm.n_owned), rows=rows)))


def run_variant(tree, mode, nts, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--tree", tree, "--reps", str(reps), "--nt"] + [str(n) for n in nts]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    for ln in out.stdout.splitlines():
        if ln.startswith("RESULT "):
            print("%s: done" % mode, flush=True)
            return json.loads(ln[7:])
    raise RuntimeError("variant %s failed:\n%s\n%s" % (mode, out.stdout[-2000:], out.stderr[-2000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--nt", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracer_coupled_timing.json"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        sys.path.insert(0, a.tree)
        worker(a.worker, a.nt, a.reps)
        return 0
    res = {}
    if a.parent_tree:
        res["parent"] = run_variant(os.path.abspath(a.parent_tree), "parent", a.nt, a.reps)
    for mode in ("per_tracer", "coupled"):
        res[mode] = run_variant(ROOT, mode, a.nt, a.reps)
    doc = dict(workload="one auxiliary solve, 100^3 eos we (16x16x2 bricks), backward Euler, GMRES(30) rtol 1e-5, block-Jacobi ILU(0)",
               reps=a.reps, variants=res)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    hdr = "%-11s %3s %10s %5s %9s %7s %10s" % ("variant", "nt", "ms/solve", "its", "launches", "reads", "ms/it")
    print(hdr)
    for mode, v in res.items():
        for r in v["rows"]:
            extra = ("  operator %.4f ms, %.1f %% of HBM peak; ILU(0) pass %.4f ms, vector kernels %.4f ms"
                     % (r["operator_ms"], 100 * r["operator_share_of_hbm_peak"], r["ilu_setup_ms"], r["vector_ms"])) if "operator_ms" in r else ""
            print("%-11s %3d %10.4f %5d %9d %7d %10.4f%s" % (mode, r["nt"], r["ms_per_solve"], r["iterations"], r["launches"],
                                                          r["scalar_reads"], r["ms_per_iteration"], extra))
    return 0


if __name__ == "__main__":
    sys.exit(main())
