/* Measurement and test entry points of libwaiwera_hip.so: kernel micro-benchmarks, HIP-event timers, launch and
 * collective counters.  NOT part of the drop-in boundary (include/waiwera_hip.h): nothing here has a counterpart in
 * the reference; bench.py, tools/ and tests/ use them. */
#ifndef WAIWERA_HIP_BENCH_H
#define WAIWERA_HIP_BENCH_H
#include "waiwera_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* collectives enqueued on this rank so far: all-reduces (Krylov inner products, flags, norms) and
 * neighbour exchanges (halos); a BiCGStab iteration costs 2 all-reduces and 2 exchanges */
int wai_comm_stats(wai_ctx *ctx, long long *allreduces, long long *exchanges);
/* gathers to a root enqueued on this rank so far (wai_gather_rows, wai_gather_fluid on more than one rank: one each; the
 * all-reduce of the row counts inside each is counted by wai_comm_stats) */
int wai_gather_stats(wai_ctx *ctx, long long *gathers);
/* kernels launched and copies enqueued by the linear-solver helpers so far (SpMV, preconditioner, vector
 * updates, reductions, halo pack / unpack, scalar read-backs): a BiCGStab iteration on one rank is 3 kernels (2 x 2 and
 * 3 x 3 blocks: the second fused launch forms its operand itself; 4 with a stored S), on several ranks 7,
 * and no copy -- every reduction is finished by the last workgroups of its producer and the residual norm is
 * posted to pinned host memory */
int wai_launch_stats(wai_ctx *ctx, long long *kernels, long long *copies);
/* tracer assembly sweeps over the faces so far: a per-tracer auxiliary solve makes nt of them, a coupled one
 * (wai_set_tracer_solve_mode) makes one */
int wai_tracer_stats(wai_ctx *ctx, long long *assembly_sweeps);

/* bench.py's A/B for the collectives' share of an iteration: on != 0 makes every all-reduce and neighbour exchange
 * of this context return without calling RCCL (results are then wrong; timing probes only).  Every rank must switch
 * together. */
int wai_bench_mute_comm(wai_ctx *ctx, int on);
/* fault injection for the tests: workgroup 0 of the following launches loses its next n partial sums of a reduction --
 * the in-launch finalisation must run into its bounded wait and the solver return KSP_DIVERGED_NANORINF (-9) */
int wai_test_drop_partials(wai_ctx *ctx, int n);
/* fault injection for the tests (negative check of the overlapped halo exchange): which = 1 -- the face bricks' launch
 * is enqueued WITHOUT waiting for the event behind the unpack on the communication stream.  Over a stream-asynchronous
 * transport a multi-rank solve must then go wrong (tests/test_hip_multirank.py); 0 restores the product's ordering */
int wai_test_drop_stream_wait(wai_ctx *ctx, int which);
/* one pass of the context's source network on the device (a network on one rank that fits LDS, else -2), whatever
 * wai_set_network_pass says, with the walk wai_set_network_walk leaves in force (k_network_pass_wave where the wave walk is
 * asked for and its schedule accepts the network, else k_network_pass): raw2n (host) = the sources' own rates [n], then their flowing enthalpies [n].
 * Returns the node states -- sources and groups 6 doubles each, reinjectors 8 each, as wai_network_evaluate -- and what
 * the pass wrote for the residual kernel: the (mode, value) pairs [2 n] and the sources' enthalpy array [n], of which the
 * pass touches the entries of the sources a reinjector feeds alone.  Out-arguments may be NULL. */
int wai_test_network_pass(wai_ctx *ctx, const double *raw2n, double *sources6, double *groups6, double *reinjectors8,
                          double *net2n, double *enth_n);
/* network passes made so far, and the stream waits the passes and the coupling build issued (either mode).  A batched
 * coupling build (wai_set_coupling_build) counts 1 + m * bs passes: the one before it and one per column */
int wai_test_network_stats(wai_ctx *ctx, long long *passes, long long *host_waits);
/* the last coupling build of wai_jacobian, whichever way it ran: kernel launches (the column loops': counted from their
 * text), columns (m * bs; 0: no build) and chunks of the batched build (0 for a column loop).  Out-arguments may be NULL */
int wai_test_coupling_build_stats(wai_ctx *ctx, long long *launches, long long *columns, long long *chunks);
/* doubles of LDS the pass on the device may take (description + raw rates + state), and what the context's network
 * takes (0: none, or one on several ranks): a network that needs more keeps the host pass.  8192 and the lane walk's need
 * under WAI_NETWORK_WALK_LANE; under WAI_NETWORK_WALK_WAVE, for a network whose topology the wave schedule accepts, 20480 and
 * the wave walk's need (staging run and schedule included) */
int wai_test_network_lds(wai_ctx *ctx, int *limit, int *needed);
/* device allocations the library holds in this process now, over all contexts and its temporaries, and their bytes: what
 * a context allocated is returned when it is destroyed, and setting something again does not grow it (tests/test_hip_memory.py) */
int wai_test_device_memory(long long *allocations, long long *bytes);
/* one preconditioned-operator application exactly as the Krylov drivers issue it, for the tests (vectors: bs * n_owned doubles,
 * host or device; scal_in / scal_out: the 16 device scalars S_RHO .. S_BREAK before / after).
 * spmv 1: z = B^-1 A (x - alpha x2) through the drivers' pc_amul (x2 may be NULL; non-NULL only where wai_pc_axpy_capable);
 * spmv 0: z = B^-1 x through pc_solve, x the partner of dot modes 2 and 4.  dot_mode 0 none, 1 (z,aux), 2 (x,z),(z,z),
 * 3 (z,z), 4 (x,z),(z,z),(x,x),(x,aux),(z,aux) -- x meaning the operand x - alpha x2.  split 1: interior bricks, then face
 * bricks (the overlapped halo exchange's two launches; one rank, meshes of seven-block rows only).  fin_phase >= -1: the
 * reductions finished (and the BiCGStab scalars of that phase derived) as the drivers finish them; -2: left as partial sums
 * and finished here by k_finalize without a derivation.  S_ALPHA is set to alpha.  A combination the library cannot serve
 * (x2 on a kernel that cannot form its operand, split without interior / face lists) is an error (-1), not a result. */
int wai_test_pc_operator(wai_ctx *ctx, int spmv, const double *x, const double *x2, double alpha, int dot_mode,
                         const double *aux, int split, int fin_phase, const double *scal_in, double *z, double *scal_out);
/* 1 when the fused preconditioned-operator launch can form its operand x - alpha x2 itself (wai_test_pc_operator's x2) */
int wai_pc_axpy_capable(wai_ctx *ctx);
/* partial sums per reduction slot the last preconditioner application (or vec_dots) left: one per brick, one per workgroup
 * of four bricks under k_pc_wave; more than 1024 means the finalisation ran in slices (tests/test_hip_fused_operator.py) */
int wai_test_partial_count(wai_ctx *ctx);
/* the brick schedule's shared descriptor tables (k_pc_park on its 16-bit column indices): returns the number of distinct
 * templates, bricks and rows the number of bricks and of template rows (24 bytes each); 0 when the schedule has none */
int wai_test_desc_templates(wai_ctx *ctx, int *bricks, int *rows);
/* short bricks packed into shared k_pc_park workgroups, for launch list `list` (0 all subdomains, 1 the interior bricks, 2 the
 * face bricks): returns the number of groups -- the workgroups of the packed launch -- as the launcher would run them now, 0
 * where it launches one workgroup per brick (nothing packs, another kernel or index form, WAI_NO_PACK); shared: the bricks
 * that share a workgroup; table: the first min(cap, 32 x groups) ints of the device's group table, per group and wave
 * {brick or -1, thread offset, first parked block, forward | backward << 16 level counts of the group} */
int wai_test_pack_groups(wai_ctx *ctx, int list, int *shared, int *table, int cap);
/* the tile schedule (wai_set_pc_tiles) of the flow system's preconditioner as set up now -- the set-up is made if it is not
 * in force -- `extended` 0: the system's own schedule (block Jacobi), 1: its extended system's (PCASM, ILU(k)).  facts[8]:
 * tiles, tile levels forward, backward, rows of the largest tile, most in-tile levels of a tile, serve (1: the sweeps run
 * k_tile_solve per tile level), row levels forward, backward (the level path's launches).  Returns the number of tiles, 0
 * where the schedule has none (no tiles set, a subdomain schedule of <= 1024 rows, sub lu, PCASM across ranks) */
int wai_test_tile_schedule(wai_ctx *ctx, int extended, int *facts);
/* one vector / reduction step of the Krylov drivers, issued through the drivers' own launchers, for the tests
 * (tests/test_hip_krylov_vec.py).  n >= 1 entries per vector, whatever the context's mesh.  vecs: seven host vectors of
 * len >= n doubles each, X R RP P V S T in this order, in and out whole (the entries behind n are guards); basis (GMRES ops):
 * (k + 1) * ld host doubles, 1 <= k <= 40 vectors ld >= n apart, in and out whole; scal: all 128 device scalars in and out
 * (0 rho, 1 rho_old, 2 alpha, 3 omega, 4 beta, 5-9 the sums S_D1 S_D2 S_DP2 S_RHONEW S_W2, 15 the breakdown code, 16 + j
 * the Gram-Schmidt coefficient h_j); post[2]: the (R,R) and breakdown code a launch posted to the host, written only where
 * the op posts.  Every partial slot is emptied first, as a driver empties them before its first producer.
 *   op (variant)
 *   DOT            S_W2 = (X, R)                                              vec_dot
 *   DOTS           0: S_D1 = (X, R), S_D2 = (P, V); 1: S_D1 alone             vec_dots + vec_finalize (host_dots)
 *   WAXPY          0: T = alpha X + R; 1: X = (w == x); 2: R = (w == y)       vec_waxpy
 *   BCGS_P / _S    P = R + beta (P - omega V) / S = R - alpha V               bcgs_update_p / bcgs_update_s
 *   BCGS_XR        X += alpha P + omega S, R = S - omega T.  0: no inner products; 1: (R,R), (R,RP) finished in the launch
 *                  (by a k_finalize launch under WAI_FIN_SEPARATE=1); 2: the same with phase 4 and the post; 3: left as
 *                  partial sums and finished here by vec_finalize                bcgs_update_xr
 *   BCGS_XRP       X, R, P in one pass                                        bcgs_update_xrp
 *   BCGS_XRP_DERIVE  the same, omega, (R,R), rho, beta derived in the launch and posted    bcgs_update_xrp_derive
 *   SCALARS        variant = phase 0, 2, 3, 4, 5 or 6 (6 posts)               bcgs_scalars
 *   MDOT           scal[16 + j] = (T, v_j), j < k                             gmres_mdot
 *   MAXPY_NORM     T -= sum h_j v_j, S_W2 = |T|^2                             gmres_maxpy_norm
 *   SCALE_TO       0: T = X / sqrt(S_W2); 1: X in place                       gmres_scale_to
 *   UPDATE_X       X += sum coef[j] v_j (coef: k host doubles; they travel through scal[64 ..])    gmres_update_x
 * n < 1, k out of range, ld < n, len < n, an unknown op or variant: -2 with the error text set, nothing launched. */
enum { WAI_KV_DOT = 0, WAI_KV_DOTS, WAI_KV_WAXPY, WAI_KV_BCGS_P, WAI_KV_BCGS_S, WAI_KV_BCGS_XR, WAI_KV_BCGS_XRP,
       WAI_KV_BCGS_XRP_DERIVE, WAI_KV_SCALARS, WAI_KV_MDOT, WAI_KV_MAXPY_NORM, WAI_KV_SCALE_TO, WAI_KV_UPDATE_X };
int wai_test_krylov_vec(wai_ctx *ctx, int op, int variant, int n, int k, long long ld, long long len, double alpha,
                        double *vecs, double *basis, const double *coef, double *scal, double *post);
/* the coarse level of the two-level preconditioner (wai_set_pc_coarse, which must be on), one piece at a time, each kernel
 * through the launcher the drivers use.  n = bs * n_owned, m = nc * bs; vectors are host or device memory, and a device
 * vector goes to the launcher as it is (so what lies behind its last entry is the caller's to check).
 *   RESTRICT      out[m] = P^T in[n]                  k_coarse_restrict
 *   GEMV          out[m] = Ac^-1 in[m]                k_coarse_gemv (sets the preconditioner up if it is not in force)
 *   PROLONG_ADD   out[n] += P in[m]                   k_coarse_prolong, the additive mode's and both modes' last launch
 *   PROLONG_SET   out[n] = P in[m]                    k_coarse_prolong, the deflated mode's first
 *   AC / AINV     out[m * m] = Ac / Ac^-1, row-major, of the set-up in force (made if there is none; 1: a pivot failed)
 *   TIMES         out[2] (host) = ms of the last set-up's Galerkin product and of its inversion, 0 unless profiling was on
 *                 (wai_profile_enable) */
enum { WAI_COARSE_RESTRICT = 0, WAI_COARSE_GEMV, WAI_COARSE_PROLONG_ADD, WAI_COARSE_PROLONG_SET, WAI_COARSE_AC, WAI_COARSE_AINV,
       WAI_COARSE_TIMES };
int wai_test_coarse(wai_ctx *ctx, int what, const double *in, double *out);
/* bytes this rank sends per halo exchange of a dof-per-cell vector, and its number of neighbours */
int wai_halo_size(wai_ctx *ctx, int dof, long long *bytes_sent, int *n_neighbours);

/* ---- measurement helpers ------------------------------------------------------------------- */
int wai_timer_start(wai_ctx *ctx);             /* hipEvent on the library's stream */
int wai_timer_stop(wai_ctx *ctx, float *ms);
/* HIP-event timed repetitions of one kernel on the library's stream (needs an assembled
 * Jacobian): which 0 block SpMV, 1 ILU(0) apply, 2 fused SpMV + ILU(0) apply + dot,
 * 3/4 timing probes of 1/2 without the substitution sweeps (generic brick kernel only), 5 one whole BiCGStab
 * iteration's launches (and collectives) back to back without the host, 6 its vector updates alone, 7 the second
 * fused launch of the iteration (operand S, or R - alpha V with WAI_BCGS_COMPOSE=1; five inner products), 9 / 10 the fused
 * kernel on the interior / the face bricks alone (the two launches of the overlapped halo exchange; 16: both as that path
 * launches them, behind one another on the compute stream), 11 .. 15 the fused
 * launch by reduction mode: 11 none, 12 (z,aux) left as partial sums, 13 (x,z),(z,z) + omega finished in the launch,
 * 14 the five merged products left as partial sums, 15 the five + omega, (R,R), rho, beta finished in the launch,
 * 17 the iteration's second fused launch exactly as it is issued on one rank (composed operand where that is the default,
 * five products, scalars and the post to the host in the launch), 18 / 19 a device-to-device copy of half the perturbed-fluid
 * scratch onto the other half (hipMemcpyAsync / a streaming copy kernel): the box's copy ceiling, 2 x bytes / time; 22 a
 * read-only stream over the whole scratch: its read ceiling; 23 z = B^-1 (A x) by the launch-per-level path (k_spmv + k_lvl_solve
 * per level) on the factor in force, for a block-Jacobi schedule of a mesh with 9 .. 16-block rows or the filled factor of fused
 * ILU(k) (the path k_pc_wide replaces),
 * 20 / 21 GMRES's Gram-Schmidt inner products / its update w -= sum h_j v_j with |w|^2 over a whole restart cycle as
 * ksp_gmres issues them, reported per Krylov iteration (needs ksp_type gmres: the basis vectors) */
int wai_bench_kernel(wai_ctx *ctx, int which, int reps, float *ms_per_launch);
/* 1 when a BiCGStab iteration's second fused launch forms its operand S = R - alpha V itself (three launches per
 * iteration, no stored S), 0 when S is a launch of its own -- for the reports' kernel names and byte counts */
int wai_bcgs_composed(wai_ctx *ctx);
/* accumulated HIP-event time (ms) and launch counts per kernel class since the last reset;
 * classes: 0 eos, 1 residual, 2 jacobian, 3 spmv, 4 pc_apply, 5 pc_setup, 6 vector, 7 transitions */
int wai_profile_enable(wai_ctx *ctx, int on);
int wai_profile_get(wai_ctx *ctx, int kclass, double *ms, long long *launches);
int wai_profile_reset(wai_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
