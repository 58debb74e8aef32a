#!/usr/bin/env python
"""Set-up and application times of the exact block solves, eos we, one Newton step's system:

    python tools/sub_lu_timing.py [--dims 32 32 8] [--brick 8 8 2] [--variants dense sublu ilu0 asm_sublu] [--out profiles/sub_lu_timing.json]

  dense      pc_type "lu": dense block inverses formed on the host at every set-up, k_lu_apply
  sublu      bjacobi + WAI_SUB_LU: k_sublu_factor / k_sublu_solve
  ilu0       bjacobi ILU(0), the fused brick kernels' factor (for scale)
  asm_sublu  asm overlap 1 + WAI_SUB_LU

Each variant is a fresh process.  Set-up (wai_pc_setup with the matrix in place: numeric phase; the symbolic phase of the
first call is reported apart, wall clock) and one application (wai_pc_apply on device arrays) are timed with the library's
HIP-event timer after two warm-ups, the median of --reps; the Krylov count is one BiCGStab solve of the step's system to
the default rtol.  A variant the library refuses is recorded with the refusal's text."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("dense", "sublu", "ilu0", "asm_sublu")


def worker(variant, dims, brick, reps):
    import numpy as np
    import torch
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation, WaiError
    g, lm, prim, region = make_case(dims=tuple(dims), brick=tuple(brick), eos="we", lens=True)
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    y = scaled(prim, region).ravel().copy()
    n = lm.n_owned * 2
    dt = 2.0e3
    assert sim.pre_eval(0.0, y) == 0
    L, f = np.zeros(n), np.zeros(n)
    sim.lhs(0.0, (0.0, 0.0), y, L)
    assert sim.residual(dt, dt, y, L, f) == 0
    assert sim.jacobian(dt, dt, y, L) == 0
    sim.set_opts(pc_type={"dense": "lu", "asm_sublu": "asm"}.get(variant, "bjacobi"), asm_overlap=1)
    if variant in ("sublu", "asm_sublu"):
        sim.set_sub_pc("lu")
    row = dict(variant=variant, cells=int(lm.n_owned), blocks=int(len(lm.sub_ptr) - 1))
    try:
        t0 = time.perf_counter()
        sim.pc_setup()
        row["first_setup_wall_s"] = time.perf_counter() - t0     # symbolic phase included
        row["kernel"] = sim.pc_kernel_name()
        dev = torch.device("cuda")
        r = torch.from_numpy(np.random.default_rng(3).normal(size=n)).to(dev)
        z = torch.zeros(n, dtype=torch.float64, device=dev)
        su, ap = [], []
        for k in range(2 + reps):
            sim.timer_start(); sim.pc_setup(); t = sim.timer_stop()
            sim.timer_start(); sim.pc_apply(r, z); u = sim.timer_stop()
            if k >= 2:
                su.append(t); ap.append(u)
        x = np.zeros(n)
        its, reason, rn = sim.ksp_solve(f, x)
        row.update(setup_ms=float(np.median(su)), setup_ms_min=float(min(su)), setup_ms_max=float(max(su)),
                   apply_ms=float(np.median(ap)), apply_ms_min=float(min(ap)), apply_ms_max=float(max(ap)),
                   krylov_iterations=int(its), krylov_reason=int(reason))
    except WaiError as e:
        row["refused"] = str(e)
    sim.destroy()
    print("RESULT " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[32, 32, 8])
    ap.add_argument("--brick", type=int, nargs=3, default=[8, 8, 2])
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=VARIANTS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sub_lu_timing.json"))
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        sys.path.insert(0, ROOT)
        worker(a.worker, a.dims, a.brick, a.reps)
        return 0
    rows = []
    for v in a.variants:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", v, "--reps", str(a.reps), "--dims"] + [str(d) for d in a.dims] + \
              ["--brick"] + [str(b) for b in a.brick]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if not got:
            raise RuntimeError("variant %s failed:\n%s\n%s" % (v, out.stdout[-2000:], out.stderr[-2000:]))
        rows.append(json.loads(got[0][7:]))
        print(rows[-1], flush=True)
    doc = {}
    if os.path.exists(a.out):
        doc = json.load(open(a.out))
    doc.setdefault("runs", []).append(dict(workload="eos we, %s cells in %s bricks, one Newton step's system" %
                                           ("x".join(map(str, a.dims)), "x".join(map(str, a.brick))), reps=a.reps, rows=rows))
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
