"""python -m waiwera_amd.run input.json [-o results.npz]

Runs a Waiwera JSON input file (the subset waiwera_amd/simulation.py covers) on the HIP path and
prints one line per accepted time step, like the reference's log of `timestep end` records.

Several ranks, one per GPU (the reference: mpiexec -np N waiwera input.json):
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 -m waiwera_amd.run input.json
every rank reads the whole input and keeps its own cells (waiwera_amd/partition.py); -o writes one file per rank
(results.rank<r>.npz: the rank's cell fields -- tracers among them -- with `owned_gid`, the cells' numbers in the one-rank
output, its sources' fields with `owned_source`, their numbers in the input, and the network's group and reinjector fields,
the same in every file).  The input's own "output.filename" is written once, by rank 0, from snapshots gathered through
the library (waiwera_amd/simulation.py); a failure to write it is rank 0's exit status."""
import argparse
import sys

from .simulation import Simulation


def _stem(path):
    """the output name without its .npz suffix (only the suffix: a '.npz' elsewhere in the path stays)"""
    import os
    root, ext = os.path.splitext(path)
    return root if ext == ".npz" else path


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m waiwera_amd.run")
    ap.add_argument("input")
    ap.add_argument("-o", "--output", default=None, help="write the final cell fields to this .npz file")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tracer-solve", choices=("per_tracer", "coupled"), default="per_tracer",
                    help="tracers: one Krylov solve each (default) or all in one solve, as the reference (bjacobi / none preconditioner)")
    ap.add_argument("--sub-lu", choices=("host", "device"), default="host",
                    help="sub-preconditioner lu under bjacobi / asm: dense block inverses from the host without overlap (default) "
                         "or the exact LU of the (overlapped) blocks on the device")
    ap.add_argument("--aux-pc", choices=("follow", "bjacobi", "asm"), default="follow",
                    help="tracer solver's preconditioner for an input without time.step.solver.auxiliary: the flow solver's "
                         "(default), bjacobi (the reference's default) or asm")
    ap.add_argument("--subdomains", choices=("chunks", "rank"), default="chunks",
                    help="the preconditioner's blocks: the mesh's chunks (default) or one block per rank, the reference's layout, "
                         "with the chunks as its tiles")
    ap.add_argument("--pc-ordering", choices=("natural", "multicolour"), default="natural",
                    help="elimination order of the flow solver's block-Jacobi ILU(0): as numbered (default, the reference's) or "
                         "multicolour (two sweep levels per block on hexahedral and MINC meshes; bjacobi with ILU(0) only)")
    ap.add_argument("--pc-coarse", choices=("additive", "deflated"), default=None,
                    help="a coarse level for the flow solver's preconditioner: piecewise constant over aggregates of cells, Galerkin, "
                         "added to (additive) or deflating (deflated) the one-level preconditioner (default: none; one rank, bjacobi or asm)")
    ap.add_argument("--coarse-aggregates", type=int, default=64,
                    help="aggregates of the coarse level, from the coordinate bisection of the cells (default 64; at most 1024 / block size)")
    ap.add_argument("--network-pass", choices=("host", "device"), default="host",
                    help="the source network's pass: on the host (default) or in one launch on the device (one rank, a network "
                         "that fits a workgroup's LDS; the same results)")
    ap.add_argument("--coupling-build", choices=("columns", "batched"), default="columns",
                    help="the Jacobian's blocks through the source network: one column at a time (default) or all columns at "
                         "once on private scratch (in force with --network-pass device; the same results)")
    ap.add_argument("--network-walk", choices=("lane", "wave"), default="lane",
                    help="how the device pass walks groups and reinjectors: one lane (default) or the whole wave (in force with "
                         "--network-pass device; networks of up to 160 KiB of LDS; the same results)")
    ap.add_argument("--cell-order", choices=("input", "compact"), default="input",
                    help="the numbering the library gets: the mesh file's, with chunks of consecutive cells as the preconditioner's "
                         "subdomains (default), or compact 3-D subdomains numbered like bricks (one rank, a mesh file, no MINC "
                         "zones; results come back in the file's numbering)")
    ap.add_argument("--subdomain-rows", type=int, default=None,
                    help="most cells of a preconditioner subdomain under either cell order, 1 to 1024 (default 512, MINC cells included)")
    a = ap.parse_args(argv)
    import os
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    kw = {}
    if world > 1:
        # the RCCL id from rank 0 to the others through the launcher's process group (the host's MPI_Bcast in the reference)
        import torch.distributed as dist
        from . import lib as wl
        dist.init_process_group(backend="gloo")
        uid = [wl.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        kw = dict(rank=rank, world=world, comm_id=uid[0])
        # one rank per GPU; WAI_BENCH_LOOPBACK=1 (tests on a one-GPU box, with a stand-in for librccl): every rank on --device
        if os.environ.get("WAI_BENCH_LOOPBACK") != "1":
            a.device = int(os.environ.get("LOCAL_RANK", a.device))
    sim = Simulation.from_json(a.input, device=a.device, tracer_solve=a.tracer_solve, sub_lu=a.sub_lu, subdomains=a.subdomains,
                               default_aux_pc=None if a.aux_pc == "follow" else a.aux_pc, pc_ordering=a.pc_ordering, network_pass=a.network_pass,
                               cell_order=a.cell_order, subdomain_rows=a.subdomain_rows,
                               coupling_build=a.coupling_build, network_walk=a.network_walk, pc_coarse=a.pc_coarse,
                               coarse_aggregates=a.coarse_aggregates, **kw)
    out = sim.run()
    if rank != 0:
        if a.output:
            sim.save(_stem(a.output) + ".rank%d.npz" % rank)
        return 0
    for (t, dt, nits, kits, tries) in sim.ts.history:
        print("timestep end: time %.6e size %.6e iterations %d linear %d tries %d" % (t, dt, nits, kits, tries))
    print("finished at t = %.6e s after %d steps" % (out["time"], sim.ts.taken))
    if a.output:
        sim.save(a.output if world == 1 else _stem(a.output) + ".rank0.npz")
    if sim.output_error is not None:
        print("error: output file not written: %s" % sim.output_error, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
