"""Times one preconditioner application z = B^-1 r (wai_pc_apply on device vectors, the device-event timer around it) on a
subdomain larger than a workgroup two ways in ONE process, alternating: with tiles set (wai_set_pc_tiles: k_tile_solve, one
launch per tile level) and with the tiles cleared (k_lvl_solve, one launch per row level: the code before tiles existed).
Two warm-up applications, then the median of 7, per path and round; the level path is also timed against itself (A/A) and
the spread of those repeats is the bar a difference has to clear.  One JSON line per case:

    python tools/pc_tiles_timing.py > profiles/pc_tiles_timing.json        # every case (216^3 needs minutes of set-up)
    python tools/pc_tiles_timing.py --small                                # 100^3 and 48 x 48 x 16 only

Cases: block Jacobi with one block per rank (sub_ptr = NULL, the reference's layout) at 216^3 and 100^3, eos we, with tiles
of 16 x 16 x 2, 16 x 8 x 4 and 8 x 8 x 8 cells (the mesh is numbered by those bricks); PCASM overlap 1 around 16 x 16 x 2
bricks at 216^3 (1152-row extended blocks; WAI_ASM_UNFUSED=1), the bricks themselves as tiles."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waiwera_amd.cases import make_case, scaled  # noqa: E402
from waiwera_amd.flow_simulation import FlowSimulation  # noqa: E402

TILES = [(16, 16, 2), (16, 8, 4), (8, 8, 8)]


class DeviceVector:
    """n doubles in device memory from the HIP runtime itself (the library takes device pointers by address)"""
    hip = None

    def __init__(self, host):
        if DeviceVector.hip is None:
            DeviceVector.hip = C.CDLL("libamdhip64.so")
        self.n, self.p = host.size, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(8 * self.n)) == 0
        assert self.hip.hipMemcpy(self.p, C.c_void_p(host.ctypes.data), C.c_size_t(8 * self.n), 1) == 0      # host to device

    def __int__(self):
        return self.p.value

    def host(self):
        out = np.empty(self.n)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(8 * self.n), 2) == 0       # device to host
        return out

    def free(self):
        self.hip.hipFree(self.p)


def median_ms(sim, r, z, warm=2, reps=7):
    for _ in range(warm):
        sim.pc_apply(r, z)
    ms = []
    for _ in range(reps):
        sim.timer_start()
        sim.pc_apply(r, z)
        ms.append(sim.timer_stop())
    return float(np.median(ms))


def launches(sim, r, z):
    k0 = sim.launch_stats()[0]
    sim.pc_apply(r, z)
    return sim.launch_stats()[0] - k0


def measure(sim, tiles, rounds=3, extended=False):
    """alternate the two paths `rounds` times; the level path twice per round (A/A)"""
    n = sim.num_dof
    r = DeviceVector(np.random.default_rng(1).normal(size=n))
    z = DeviceVector(np.zeros(n))
    out = dict(tiles_ms=[], levels_ms=[], levels_again_ms=[])
    for _ in range(rounds):
        sim.set_pc_tiles(tiles)
        assert sim.pc_setup() == 0
        out["tiles_ms"].append(median_ms(sim, r, z))
        out["tiles_kernel"] = sim.pc_kernel_name()
        out["tiles_launches"] = launches(sim, r, z)
        out["schedule"] = sim.tile_schedule(extended=extended)
        sim.synchronize()
        zt = z.host()
        sim.set_pc_tiles(None)
        assert sim.pc_setup() == 0
        out["levels_ms"].append(median_ms(sim, r, z))
        out["levels_again_ms"].append(median_ms(sim, r, z))
        out["levels_kernel"] = sim.pc_kernel_name()
        out["levels_launches"] = launches(sim, r, z)
        sim.synchronize()
        out["same_bits"] = bool(np.array_equal(zt, z.host()))
    lv = np.array(out["levels_ms"] + out["levels_again_ms"])
    out["levels_spread"] = float((lv.max() - lv.min()) / np.median(lv))      # A/A: the level path against itself
    out["ratio_levels_over_tiles"] = float(np.median(lv) / np.median(out["tiles_ms"]))
    r.free(); z.free()
    return out


def system(dims, brick, one_block, pc):
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos="we", lens=True)
    tiles = np.asarray(lm.sub_ptr, dtype=np.int32).copy()
    if one_block:
        lm.sub_ptr = None
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    sim.set_opts(pc_type=pc, asm_overlap=1, ilu_levels=0)
    sim.setup_jacobian()
    y = scaled(prim, region, "we").ravel().copy()
    L = np.zeros(sim.num_dof)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, 1.0, y, L)
    assert sim.jacobian(0.0, 5.0e4, y, L) == 0
    return sim, tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="without the 216^3 cases")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiles", default="0,1,2", help="which of the tile shapes 16x16x2, 16x8x4, 8x8x8 (indices)")
    ap.add_argument("--no-asm", action="store_true", help="without the PCASM case")
    ap.add_argument("--no-bjacobi", action="store_true", help="without the one-block-per-rank cases")
    a = ap.parse_args()
    sizes = [(100, 100, 100), (48, 48, 16)] if a.small else [(216, 216, 216), (100, 100, 100)]
    for dims in ([] if a.no_bjacobi else sizes):
        for brick in [TILES[int(i)] for i in a.tiles.split(",")]:
            sim, tiles = system(dims, brick, True, "bjacobi")
            row = dict(case="one block per rank", pc="bjacobi", dims=dims, tile=brick, n=sim.num_dof // 2)
            row.update(measure(sim, tiles, a.rounds))
            print(json.dumps(row), flush=True)
            sim.destroy()
    if a.no_asm:
        return
    os.environ["WAI_ASM_UNFUSED"] = "1"
    dims = (48, 48, 16) if a.small else (216, 216, 216)
    sim, tiles = system(dims, (16, 16, 2), False, "asm")
    row = dict(case="asm overlap 1, unfused", pc="asm", dims=dims, tile=(16, 16, 2), n=sim.num_dof // 2)
    row.update(measure(sim, tiles, a.rounds, extended=True))
    print(json.dumps(row), flush=True)
    sim.destroy()


if __name__ == "__main__":
    main()
