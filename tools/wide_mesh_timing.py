#!/usr/bin/env python
"""Timing of the wide-row preconditioned operator on a mesh of about 2 M cells whose cells have up to 14 faces.

    python tools/wide_mesh_timing.py [--motifs 52 52] [--layers 10] [--eos we wce] [--out profiles/wide_mesh_timing.json]

The plan is a tiling of 3 x 3 motifs of coarse squares: the centre square stays coarse, its eight neighbours are
refined 3 x 3, so every centre column borders twelve fine columns (the mesh of tests/wide_mesh.py, repeated).  The
mesh is built in numpy, face by face type, without the per-cell loop of unstructured.build_mesh.  For each EOS, on
the device's own FD Jacobian with block-Jacobi ILU(0) on subdomains of 512 consecutive cells:
  - one application z = B^-1 (A x) by k_pc_wide (wai_bench_kernel 11) and by the launch-per-level path it replaces on
    the same factor (k_spmv + k_lvl_solve per level, wai_bench_kernel 23), HIP-event timed after warm-up;
  - a BiCGStab solve of J x = -f, HIP-event timed, per Krylov iteration;
  - the algorithmic bytes of k_pc_wide and the % of the 8 TB/s peak they reach."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
GRAV = -9.8


def motif_plan(mx, my, h):
    """columns of the tiled plan: (centroid xy (C, 2), area (C,), lateral faces (c1, c2, normal axis, sign, d1, d2,
    length, face centroid xy)); motif m = (mj, mi) holds its 72 fine columns, then its coarse centre"""
    d = h / 3.0
    local = -np.ones((9, 9), dtype=np.int64)
    k = 0
    for b in range(9):
        for a in range(9):
            if not (3 <= a <= 5 and 3 <= b <= 5):
                local[a, b] = k
                k += 1
    FX, FY = 9 * mx, 9 * my
    A, B = np.meshgrid(np.arange(FX), np.arange(FY), indexing="ij")
    fine = local[A % 9, B % 9] >= 0
    colid = -np.ones((FX, FY), dtype=np.int64)
    colid[fine] = ((B[fine] // 9) * mx + A[fine] // 9) * 73 + local[A[fine] % 9, B[fine] % 9]
    nm = mx * my
    ncol = 73 * nm
    cxy = np.zeros((ncol, 2))
    area = np.full(ncol, d * d)
    cxy[colid[fine], 0] = (A[fine] + 0.5) * d
    cxy[colid[fine], 1] = (B[fine] + 0.5) * d
    mi, mj = np.arange(nm) % mx, np.arange(nm) // mx
    centre = np.arange(nm) * 73 + 72
    cxy[centre, 0] = (9 * mi + 4.5) * d
    cxy[centre, 1] = (9 * mj + 4.5) * d
    area[centre] = h * h
    faces = []
    # fine-fine faces along x and along y
    for axis in (0, 1):
        if axis == 0:
            a1, b1 = A[:-1, :], B[:-1, :]
            a2, b2 = a1 + 1, b1
        else:
            a1, b1 = A[:, :-1], B[:, :-1]
            a2, b2 = a1, b1 + 1
        c1, c2 = colid[a1, b1], colid[a2, b2]
        ok = (c1 >= 0) & (c2 >= 0)
        c1, c2 = c1[ok], c2[ok]
        fxy = 0.5 * (cxy[c1] + cxy[c2])
        faces.append((c1, c2, np.full(c1.size, axis), np.ones(c1.size), np.full(c1.size, 0.5 * d), np.full(c1.size, 0.5 * d),
                      np.full(c1.size, d), fxy))
    # centre - fine faces: three per side
    for axis, sign, da, db in ((0, -1, -1, None), (0, 1, 3, None), (1, -1, None, -1), (1, 1, None, 3)):
        for t in range(3):
            if axis == 0:
                fa, fb = 9 * mi + 3 + da, 9 * mj + 3 + t
            else:
                fa, fb = 9 * mi + 3 + t, 9 * mj + 3 + db
            c2 = colid[fa, fb]
            fxy = cxy[c2].copy()
            fxy[:, axis] -= sign * 0.5 * d
            faces.append((centre, c2, np.full(nm, axis), np.full(nm, float(sign)), np.full(nm, 1.5 * d), np.full(nm, 0.5 * d),
                          np.full(nm, d), fxy))
    cat = [np.concatenate([f[q] for f in faces]) for q in range(8)]
    return cxy, area, cat


def tiled_wide_mesh(mx, my, layers, h=90.0, dz=50.0, chunk=512):
    """LocalMesh of the tiled plan in `layers` layers (layer-major cell order), a top Dirichlet boundary, four sources"""
    from waiwera_amd.mesh import LocalMesh, default_rock
    cxy, area, (l1, l2, lax, lsg, ld1, ld2, llen, lfxy) = motif_plan(mx, my, h)
    ncol = cxy.shape[0]
    n = ncol * layers
    nlat = l1.size
    lay = np.repeat(np.arange(layers), nlat)
    zc = -(np.arange(layers) + 0.5) * dz
    rec = []
    # lateral faces, every layer
    r = np.zeros((nlat * layers, 12))
    r[:, 0] = np.tile(llen, layers) * dz
    r[:, 1], r[:, 2] = np.tile(ld1, layers), np.tile(ld2, layers)
    r[:, 3] = r[:, 1] + r[:, 2]
    ax, sg = np.tile(lax, layers), np.tile(lsg, layers)
    r[np.arange(r.shape[0]), 4 + ax] = sg
    r[:, 8:10] = np.tile(lfxy, (layers, 1))
    r[:, 10] = zc[lay]
    r[:, 11] = ax + 1
    fc = [np.stack([np.tile(l1, layers) + lay * ncol, np.tile(l2, layers) + lay * ncol], axis=1)]
    rec.append(r)
    # vertical faces between layers: upper cell first, normal -z
    lv = np.repeat(np.arange(layers - 1), ncol)
    cc = np.tile(np.arange(ncol), layers - 1)
    r = np.zeros((cc.size, 12))
    r[:, 0] = area[cc]
    r[:, 1] = r[:, 2] = 0.5 * dz
    r[:, 3] = dz
    r[:, 6] = -1.0
    r[:, 7] = GRAV * -1.0
    r[:, 8:10] = cxy[cc]
    r[:, 10] = -(lv + 1) * dz
    r[:, 11] = 3
    fc.append(np.stack([lv * ncol + cc, (lv + 1) * ncol + cc], axis=1))
    rec.append(r)
    # top boundary: the top layer's cells, ghost cells n .. n + ncol
    r = np.zeros((ncol, 12))
    r[:, 0] = area
    r[:, 1] = r[:, 3] = 0.5 * dz
    r[:, 6] = 1.0
    r[:, 7] = GRAV
    r[:, 8:10] = cxy
    r[:, 11] = 3
    fc.append(np.stack([np.arange(ncol), n + np.arange(ncol)], axis=1))
    rec.append(r)
    m = LocalMesh(dims=(n, 1, 1), spacing=(0.0, 0.0, 0.0), part=(1, 1, 1), rank=0, brick=(chunk, 1, 1), n_global=n)
    m.n_owned, m.n_halo, m.n_bc = n, 0, ncol
    m.face_cells = np.concatenate(fc).astype(np.int32)
    m.face_geom = np.concatenate(rec)
    m.n_faces = m.face_cells.shape[0]
    cg = np.zeros((n + ncol, 4))
    cg[:n, :2] = np.tile(cxy, (layers, 1))
    cg[:n, 2] = np.repeat(zc, ncol)
    cg[:n, 3] = np.tile(area, layers) * dz
    cg[n:, :2] = cxy
    m.cell_geom = cg
    m.rock = np.tile(default_rock(1)[0], (n + ncol, 1))
    m.bc_region = np.ones(ncol, dtype=np.int32)
    m.sub_ptr = np.append(np.arange(0, n, chunk), n).astype(np.int32)
    m.owned_gid = np.arange(n)
    m.nbr_ranks = np.zeros(0, dtype=np.int32)
    m.send_ptr = np.zeros(1, dtype=np.int32)
    m.send_idx = np.zeros(0, dtype=np.int32)
    m.recv_ptr = np.zeros(1, dtype=np.int32)
    src = np.array([n // 5, 2 * n // 5, 3 * n // 5, 4 * n // 5]) + ncol
    m.n_src = src.size
    m.src_cell = src.astype(np.int32)
    m.src_rate = np.array([-5.0, -5.0, -5.0, 5.0])
    m.src_enthalpy = np.array([0.0, 0.0, 0.0, 1.0e5])
    m.src_component = np.array([0, 0, 0, 1], dtype=np.int32)
    return m


def initial_state(m, eos):
    from waiwera_amd.mesh import liquid_density_estimate
    n = m.n_owned
    depth = -m.cell_geom[:n, 2]
    T = 20.0 + 0.05 * depth
    P = 1.0e5 + 9.8 * liquid_density_estimate(T) * depth
    top = {"we": [1.0e5, 20.0], "wce": [1.0e5, 20.0, 0.02e5]}[eos]
    prim = np.zeros((n, len(top)))
    prim[:, 0], prim[:, 1] = P, T
    if eos == "wce":
        prim[:, 2] = 0.02 * P
    m.bc_primary = np.tile(np.asarray(top), (m.n_bc, 1))
    return prim, np.ones(n, dtype=np.int32)


def measure(m, eos, reps):
    from waiwera_amd.cases import scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    prim, region = initial_state(m, eos)
    sim = FlowSimulation(m, eos=eos)
    sim.set_regions(region)
    bs = sim.num_primary_variables
    y = np.ascontiguousarray(scaled(prim, region, eos).ravel())
    n = sim.num_dof
    dt = 1.0e5
    L, f = np.zeros(n), np.zeros(n)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, dt, y, L)
    sim.residual(0.0, dt, y, L, f)
    assert sim.jacobian(0.0, dt, y, L) == 0
    assert sim.pc_setup() == 0
    name = sim.pc_kernel_name()
    fused = sim.bench_kernel(11, reps)
    level = sim.bench_kernel(23, reps)
    sim.set_opts(ksp_type="bcgs", ksp_rtol=1e-8)
    x = np.zeros(n)
    sim.ksp_solve(-f, x)                    # warm-up solve
    x[:] = 0.0
    sim.timer_start()
    its, reason, rn = sim.ksp_solve(-f, x)
    ms_solve = sim.timer_stop()
    nnzb = int(len(sim.jacobian_values()) // (bs * bs))
    N = m.n_owned
    nbytes = nnzb * (16 * bs * bs + 4) + N * (16 + 2 * 8 * bs)
    out = dict(eos=eos, bs=bs, cells=N, nnzb=nnzb, blocks_per_row=nnzb / N, max_faces=int(np.bincount(m.face_cells.ravel())[:N].max()),
               kernel=name, k_pc_wide_ms=fused, level_path_ms=level, speedup_vs_level_path=level / fused,
               algorithmic_bytes=nbytes, bytes_per_block_row=nbytes / N, k_pc_wide_pct_of_peak=100.0 * nbytes / (fused * 1e-3) / PEAK,
               bcgs_iterations=its, bcgs_reason=reason, bcgs_ms=ms_solve, bcgs_ms_per_iteration=ms_solve / max(its, 1))
    sim.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--motifs", type=int, nargs=2, default=[52, 52])
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--eos", nargs="+", default=["we", "wce"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.time()
    m = tiled_wide_mesh(a.motifs[0], a.motifs[1], a.layers)
    build_s = time.time() - t0
    res = dict(command="python tools/wide_mesh_timing.py " + " ".join(sys.argv[1:]), mesh_build_s=build_s,
               peak_bytes_per_s=PEAK, results=[measure(m, e, a.reps) for e in a.eos])
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
