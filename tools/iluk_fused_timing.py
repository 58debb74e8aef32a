"""Times one preconditioned-operator application z = B^-1 (A x) under block-Jacobi ILU(k) three ways on the same matrix:
the fused launch (k_pc_wide on the filled factor, wai_bench_kernel 2), the launch-per-level path on the same factor
(wai_bench_kernel 23) and, beside them, ILU(0) on the brick kernels.  One JSON line per case:

    python tools/iluk_fused_timing.py > profiles/iluk_fused_kernels.json
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waiwera_amd.cases import make_case, scaled  # noqa: E402
from waiwera_amd.flow_simulation import FlowSimulation  # noqa: E402

# (eos, dims, brick, ILU level): 2 x 2 blocks in the bench's bricks (staged form), ILU(2) there (16 blocks per row: the
# parked form), 3 x 3 blocks in one-wave bricks (parked form)
CASES = [("we", (100, 100, 100), (16, 16, 2), 1), ("we", (100, 100, 100), (16, 16, 2), 2), ("wce", (64, 64, 64), (8, 4, 2), 1)]


def main():
    for eos, dims, brick, levels in CASES:
        g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=True)
        sim = FlowSimulation(lm, eos=eos)
        sim.set_regions(region)
        sim.set_opts(pc_type="bjacobi", ilu_levels=levels)
        y = scaled(prim, region, eos).ravel().copy()
        L = np.zeros(sim.num_dof)
        assert sim.pre_eval(0.0, y) == 0
        sim.lhs(0.0, 1.0, y, L)
        assert sim.jacobian(0.0, 5.0e4, y, L) == 0
        assert sim.pc_setup() == 0
        row = dict(eos=eos, dims=dims, brick=brick, ilu_levels=levels, bricks=len(lm.sub_ptr) - 1, kernel=sim.pc_kernel_name(),
                   fused_ms=sim.bench_kernel(2, reps=50), fused_solve_only_ms=sim.bench_kernel(1, reps=50),
                   level_path_ms=sim.bench_kernel(23, reps=20), spmv_ms=sim.bench_kernel(0, reps=50))
        sim.set_opts(ilu_levels=0)
        assert sim.pc_setup() == 0
        row.update(ilu0_kernel=sim.pc_kernel_name(), ilu0_fused_ms=sim.bench_kernel(2, reps=50))
        print(json.dumps(row), flush=True)
        sim.destroy()


if __name__ == "__main__":
    main()
