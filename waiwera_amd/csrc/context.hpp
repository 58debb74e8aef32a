// Internal context of libwaiwera_hip.so: device-resident mesh, fluid state, BCSR Jacobian,
// preconditioner schedule and Krylov work vectors.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/waiwera_hip.h"
#include "coarse_space.hpp"   // CoarseSpace
#include "colour_order.hpp"   // ColourFacts
#include "coupling_batch.hpp" // CouplingBatch
#include "devbuf.hpp"
#include "ilu_schedule.hpp"   // ScheduleFacts
#include "mesh_pattern.hpp"   // MAX_CELL_FACES
#include "network_pass.hpp"   // NetFlatHost
#include "network_wave.hpp"   // NetWaveHost
#include "physics.hip.h"
#include "tile_schedule.hpp"  // TileFacts

namespace wai {

// Element (s, r, k) of block row i in a block-ELL value array of n block rows (layout rationale:
// linalg_device.hip.h, "Matrix entry addressing").
// The stride between the element planes of block sizes >= 3 is not n but n rounded up to 512 doubles (4 KB), and never a
// multiple of 2 MB: how a slot's nine planes fall onto the memory channels depends on it.  MEASURED (C4's SpMV alone,
// tools/micro/spmv3_stride.hip, nine strides x three fresh allocations on one box): stride n = 5 029 280 doubles
// 71.8-72.3 % of HBM peak, a multiple of 2 MB 70.0-72.9 %, 4-KB multiples with 0-132 KB added 71.4-78.2 % (mean 75 %).
// Every array indexed through ell_ix with bs >= 3 is allocated with ell_rows(bs, n) rows.
__host__ __device__ __forceinline__ size_t ell_ld(size_t n) {
  size_t ld = (n + 511) & ~(size_t)511;
  if ((ld & 262143) == 0) ld += 512;
  return ld;
}
__host__ __device__ __forceinline__ size_t ell_rows(int bs, size_t n) {
  if (bs >= 3) return ell_ld(n);
  return n;
}
// Block sizes >= 3: SELL-64 in slices of eight slots (round 5).  The bs^2 elements of 64 consecutive block rows of slot s
// sit together, and the (up to) eight slots of those 64 rows follow one another: everything a wave reads of its 64 rows --
// 7 slots x 9 elements x 512 B = 32 KB for the 7-point stencil of 3 x 3 blocks -- is ONE contiguous run (the eighth
// slot's 4.6 KB are a hole nobody reads).  With one stream per slot, C4's k_spmv<3> ran at 64 % of HBM peak on one box
// and 74-76 % on others, and between 72.6 and 85.5 % in eight processes on one box; SELL-64 measured 76.0 % in ten
// processes out of ten.  The earlier layouts (one plane per element, one stream per slot, block rows) live on in
// tools/micro/spmv3_variants.hip (profiles/spmv3_variants_r4.log).  Slot s of block row i, element e = r bs + k:
//     (s / 8) * 8 bs^2 ld  +  (((i / 64) * 8 + s % 8) * bs^2 + e) * 64  +  i % 64,      ld = ell_ld(n)
// so wider systems (ILU(k) fill: W > 8) take further slices of eight.  An array of ONE block per row (the inverted
// pivots) keeps the per-slot form through ell_ix1.  Arrays indexed through ell_ix are allocated with ell_size doubles.
// Block sizes 1 and 2: the block rows of a plane per (slot, row-in-block), element i of a plane the bs-vector of block row i.
__host__ __device__ __forceinline__ size_t ell_ix1(int bs, size_t n, int r, int k, size_t i) {
  if (bs >= 3) return ((i >> 6) * (size_t)(bs * bs) + (size_t)(r * bs + k)) * 64 + (i & 63);
  return ((size_t)r * n + i) * bs + k;
}
__host__ __device__ __forceinline__ size_t ell_ix(int bs, size_t n, int s, int r, int k, size_t i) {
  if (bs >= 3) {
    const size_t bb = (size_t)(bs * bs);
    return (size_t)(s >> 3) * 8 * bb * ell_ld(n) + ((((i >> 6) << 3) + (size_t)(s & 7)) * bb + (size_t)(r * bs + k)) * 64 + (i & 63);
  }
  // (2 x 2 blocks: the two block rows of 64 rows together inside a slot, the same idea, MEASURED without effect -- C3's
  // fused launch 0.5326 / 0.5406 / 0.5387 against 0.5409 / 0.5713 / 0.5388 ms, the 108^3 share 0.0826 against 0.0820;
  // profiles/group2_ab_r4.log -- two planes per slot are few enough)
  return ((size_t)(s * bs + r) * n + i) * bs + k;
}
// doubles of a W-slot array indexed through ell_ix
__host__ __device__ __forceinline__ size_t ell_size(int bs, size_t n, int W) {
  if (bs >= 3) return (size_t)((W + 7) / 8) * 8 * bs * bs * ell_ld(n);
  return (size_t)W * bs * bs * ell_rows(bs, n);
}

enum KClass { KC_EOS = 0, KC_RESIDUAL = 1, KC_JACOBIAN = 2, KC_SPMV = 3, KC_PC_APPLY = 4,
              KC_PC_SETUP = 5, KC_VECTOR = 6, KC_TRANSITIONS = 7, KC_COUNT = 8 };

// device scalars of the Krylov solvers (Krylov::scal) and the reduction slots of the same numbers (Krylov::partials)
enum { S_RHO = 0, S_RHOOLD = 1, S_ALPHA = 2, S_OMEGA = 3, S_BETA = 4, S_D1 = 5, S_D2 = 6,
       S_DP2 = 7, S_RHONEW = 8, S_W2 = 9, S_BREAK = 15, S_H = 16 };

// The inner products a preconditioned-operator application (launch_pc, pc_solve, pc_amul) reduces as it computes
// z = B^-1 (A in) or z = B^-1 in, chosen by its dot mode.  A mode's products go to consecutive reduction slots, from
// pc_dot_slot0(mode) on, in this order:
//   PC_DOT_NONE   0  none
//   PC_DOT_ZA     1  (z, aux)                                          S_D1
//   PC_DOT_XZ     2  (in, z), (z, z)                                   S_D1, S_D2
//   PC_DOT_ZZ     3  (z, z)                                            S_DP2
//   PC_DOT_MERGED 4  (in, z), (z, z), (in, in), (in, aux), (z, aux)    S_D1, S_D2, S_DP2, S_RHONEW, S_W2
// Mode 4 is BiCGStab's merged reductions (krylov.hip, bcgs_second_half): one application, five inner products.
enum PcDot { PC_DOT_NONE = 0, PC_DOT_ZA = 1, PC_DOT_XZ = 2, PC_DOT_ZZ = 3, PC_DOT_MERGED = 4 };
static_assert(S_D2 == S_D1 + 1 && S_DP2 == S_D1 + 2 && S_RHONEW == S_D1 + 3 && S_W2 == S_D1 + 4,
              "the merged reductions' slots S_D1 .. S_W2 are consecutive: a reduction addresses them as slot0 + index");
__host__ __device__ constexpr int pc_dot_slot0(int mode) { return mode == PC_DOT_ZZ ? S_DP2 : S_D1; }
__host__ __device__ constexpr int pc_dot_nslots(int mode) {
  return mode == PC_DOT_MERGED ? 5 : (mode == PC_DOT_XZ ? 2 : (mode == PC_DOT_NONE ? 0 : 1));
}

struct Comm;  // RCCL state (comm.cpp)

struct DeviceMesh {
  int n_owned = 0, n_halo = 0, n_bc = 0, n_prim = 0, n_local = 0, n_faces = 0, max_deg = 0;
  DevBuf<double> rock;       // SoA 8 x n_local
  DevBuf<double> vol;        // n_local
  DevBuf<double> fgeom;      // SoA 5 x n_faces: area, d1, d2, d12, g.n
  DevBuf<int> fdir;          // permeability direction 1..3
  // ELL cell->face adjacency of owned cells, slot-major: [slot * n_owned + cell]
  DevBuf<int> adj_face;   // face*2 + side (side 0: cell is cell 1 of the face), -1 = empty
  DevBuf<int> adj_other;  // local index of the cell across the face
  DevBuf<int> adj_blk;    // matrix slot of (cell, other) in the cell's block row, -1 for a bc cell
  DevBuf<int> adj_tblk;   // matrix slot of (other, cell) in the OTHER cell's block row, -1 where the other cell is no owned row (k_jacobian_sym)
  DevBuf<int> diag_blk;   // matrix slot of (cell, cell)
  DevBuf<int> cell_src;   // first source in the cell or -1
  DevBuf<int> face_cells; // [2 n_faces] (cell 1, cell 2) of every face: flux output only
};

struct Sources {
  int n = 0;
  DevBuf<int> cell, comp, pcomp, next;   // pcomp: production components (wai_set_source_production_component), 0: none
  DevBuf<double> rate, enth;
  DevBuf<SrcCtl> ctl;      // state-dependent controls (wai_set_source_controls), null: none
  DevBuf<double> net;      // [2 n] what the source network does to each source (source_network_rate), null: no network
};

// Source network: groups and reinjectors (src/source_network_group.F90, source_network_reinjector.F90),
// evaluated between the EOS sweep and the residual kernel of every residual evaluation, as source_network%update is
// (src/source_network.F90:90-130) -- on the host unless wai_set_network_pass asks for the device.  One description
// (flat: network_pass.hpp, built and validated by build_net_flat) and one pass (network_pass) serve both places; what is
// kept of a pass is one run of doubles (net_state_keep: the six flow values of source_network_node_type per source and
// group, eight doubles per reinjector), h_state on the host and d_state on the device.
struct Network {
  bool on = false;
  // flat: the description, numbered by global source index where the network spans several ranks.  Its doubles carry the
  // sources' separators and specified enthalpies (h_ctl, h_enth0): flat_gen counts their changes, flat_host_gen /
  // flat_dev_gen say which of them flat.dw and the device's copy hold (network_flat_refresh, network_flat_upload).
  // flat_fits: description and state fit a workgroup's static LDS (one rank only: the pass on the device)
  NetFlatHost flat;
  int flat_gen = 1, flat_host_gen = 0, flat_dev_gen = 0;
  bool flat_fits = false;
  std::vector<double> h_enth0, h_raw;              // per source: specified enthalpies; raw rates, then enthalpies (2 n)
  std::vector<SrcCtl> h_ctl;                       // host copy of the control records (separators)
  // the host pass: its working state (net_state_carve), what it hands over per source of the network -- (mode, value)
  // pairs and the fed sources' enthalpies -- and the state kept of the last pass, host or device (network_fetch_state)
  std::vector<double> h_work, h_net, h_enth, h_state;
  DevBuf<double> d_raw;                            // device scratch: raw rates and enthalpies, 2 n
  // A network whose sources live on several ranks (source_network_group.F90:494-515, 579-596: gathers over the
  // group's communicator): every rank holds the whole description, numbered by GLOBAL source index; the sources' own
  // rates are all-gathered (an all-reduce of a vector each rank fills at its own entries) before the pass, which
  // every rank then evaluates identically.  gidx: global index of each local source (none on a rank without sources);
  // n_global: the sources of all ranks, 0: one rank, identity
  std::vector<int> gidx;
  int n_global = 0;
  DevBuf<double> d_all;                            // [2 n_global] all-reduce buffer
  std::vector<double> h_loc, l_net, l_enth;        // local staging: raw rates (2 n_local), factors (2 n_local), enthalpies
  // Jacobian couplings through the network (flow_simulation_modify_jacobian, src/flow_simulation.F90:3023-3084,
  // dependencies of src/source_network.F90:359-498): blocks E[i][j] = d R(cell i) / d y(cell j) *through the
  // network pass* for the cells of the network's sources (the reference inserts the outer product of its
  // dependency rows and columns; pairs without a dependence difference to exact zeros), by the FD rule of
  // the Jacobian.  The operator is A + E; the preconditioner is built from A.
  std::vector<int> h_cell;                         // cell of every source
  bool coupling = true;                            // wai_set_network_couplings
  bool cp_in_pc = true;                            // ... and inside the preconditioner's ILU pattern (wai_set_network_couplings 2; one rank)
  bool cp_valid = false;                           // E belongs to the Jacobian in force and has a nonzero entry
  std::vector<int> cp_cells;                       // distinct (local) cells of the network's sources, ascending
  std::vector<double> h_cp_val;                    // [ml][m][bs][bs] row-major, ml = cp_cells.size() rows, m columns
  // a network on several ranks: the columns are the network's cells of ALL ranks, ordered by (owner rank, local
  // cell) -- this rank's cells are the columns cp_j0 .. cp_j0 + ml; one rank: m = ml, cp_j0 = 0
  bool cp_span = false;
  int cp_m = 0, cp_j0 = 0;
  std::vector<int> cp_owner;                       // [m] owner rank of every column cell
  DevBuf<int> d_cp_cells;
  DevBuf<double> d_cp_val, d_cp_f, d_cp_g;
  DevBuf<double> d_cp_x;                           // [m * bs + 2] x at the column cells, gathered over the ranks
  // The pass on the device (wai_set_network_pass; k_network_pass of kernels_network.hip): the description's two arrays
  DevBuf<int> d_flat_iw;
  // The wave-wide walk (wai_set_network_walk; network_wave.hpp): its schedule, built with the flat description whatever walk
  // is asked for.  wave_built: the topology was accepted (the schedule's lists and its need of LDS stand); wave_ok: and the
  // need fits 160 KiB; wave_err: why not
  NetWaveHost wave;
  bool wave_built = false, wave_ok = false;
  std::string wave_err;
  DevBuf<int> d_wave_ww;
  DevBuf<double> d_flat_dw;
  DevBuf<double> d_state;                          // what the last device pass kept (net_state_keep)
  bool state_on_device = false;                    // ... is newer than h_state (network_fetch_state)
  bool enth_stale = false;                         // the host pass hands the device every fed source's enthalpy again
  DevBuf<double> d_cp_yh;                          // coupling build on the device: y_jk and h of the column in hand
  DevBuf<int> d_cp_flag;                           // ... an entry of E is nonzero
  bool cp_on_device = false;                       // d_cp_val is newer than h_cp_val (network_fetch_couplings)
  // the batched coupling build (wai_set_coupling_build; coupling_batch.hpp): one chunk's columns of private scratch,
  // allocated by the first batched build and kept while it is large enough
  DevBuf<double> d_cb_scratch;
  long long cb_doubles = 0;                        // ... its size
};

// Block matrix in HBM: block-ELL, slot-major struct-of-arrays ("SELL" with one slice):
//   col[s*n + i]            column of slot s of block row i (padding slots: col = i, values 0)
//   val[(s*bb + e)*n + i]   entry e (row-major inside the bs x bs block) of that block
// Slots of a row are in ascending column order, i.e. slot s of row i is BCSR block
// rowptr[i] + s: the BCSR arrays (rowptr / colidx on the host) remain the exchange format of
// the C ABI, the device layout is what lets one-thread-per-row kernels read and write fully
// coalesced (64 consecutive doubles per wave instruction).
// A Bcsr is a VIEW handed to the launchers: it owns nothing.  The three systems on the mesh's pattern (LinSys below)
// share n, ncols, nnzb, W, col and rowptr (wai_ctx::pat) and differ in bs, val, dg and fdg; an extended ASM system's E
// has a pattern of its own (AsmSystem).  The owners stand beside the views: Pattern's col and rowptr, LinSys' val and fdg,
// AsmSystem's E_col and E_val.
struct Bcsr {
  int n = 0, ncols = 0, nnzb = 0, bs = 0, W = 0;
  int* col = nullptr;
  double* val = nullptr;
  int* rowptr = nullptr;  // device copy of the BCSR row pointer (layout conversion kernels)
  // dg > 0: the coupled tracer system (kernels_tracer_block.hip) -- dg independent scalar matrices on this ONE set of
  // column planes, i.e. diagonal dg x dg blocks stored as their diagonals: val[(slot * dg + t) * n + row], vectors
  // interleaved [row][t].  fdg: its ILU(0) factor in the same layout (diagonal slot: the inverted pivot)
  int dg = 0;
  double* fdg = nullptr;
};
// The sparsity pattern of the mesh (the cell itself and its neighbours among the owned and ghost cells), single and shared:
// built once (wai_ctx_create) and owned here; every LinSys' matrix is a view on it
struct Pattern {
  int n = 0, ncols = 0, nnzb = 0, W = 0;
  DevBuf<int> col;        // block-ELL column planes [W][n]
  DevBuf<int> rowptr;     // device copy of h_rowptr
  std::vector<int> h_rowptr, h_colidx;
};

struct LinSys;
// The tile schedule of a big IluSchedule (wai_set_pc_tiles; tile_schedule.hpp, where build_tile_schedule makes the facts and
// every table on the host): the tables on the device.  n_tiles = 0 and null tables: the schedule has no tiles
struct TileTables : TileFacts {
  DevBuf<int> tile_ptr;     // [n_tiles + 1] row ranges
  DevBuf<int> tile_nin;     // [n_tiles] in-tile levels: forward | backward << 16
  DevBuf<int> ord_f, ord_b; // tiles sorted by forward / backward tile level (tile ranges of each level: tl_f_ptr / tl_b_ptr)
  DevBuf<int> row_lev;      // [n] in-tile level of the row: forward | backward << 16
  void clear() {
    static_cast<TileFacts&>(*this) = TileFacts();
    tile_ptr.reset(); tile_nin.reset(); ord_f.reset(); ord_b.reset(); row_lev.reset();
  }
};
// Block-Jacobi ILU(0): one workgroup per subdomain, one thread per block row.  The facts (sizes, extremes, the flags the
// kernel selection reads, the host copy `sub` of sub_ptr, the level sets' row ranges) are ScheduleFacts' (ilu_schedule.hpp,
// where build_host_schedule makes them and every table on the host); here are the tables on the device.
struct IluSchedule : ScheduleFacts {
  DevBuf<int> sub_ptr;      // nsub+1 row ranges
  DevBuf<int> sub_nlev;     // per subdomain: forward levels | backward levels << 16
  DevBuf<int> sub_split;    // per subdomain: leading rows longer than half the block-ELL width (k_pc_rows: MINC bricks), or null
  DevBuf<int> row_info;     // per row: lfirst | dslot<<4 | ulast<<8 | lev_f<<12 | lev_b<<22 (big, wide: lfirst | dslot<<8 | ulast<<16)
  DevBuf<unsigned long long> row_infow;   // wide: the 64-bit descriptor
  DevBuf<double> fval;      // factor in the matrix' block-ELL layout; the diagonal slot holds
                            // the inverted pivot block
  DevBuf<double> dinv;      // inverted pivot blocks, SoA [bb][n]
  DevBuf<int> row_uoff;     // first parked upper block of a row inside its subdomain
  DevBuf<int> row_tslot;    // per row: slot of A_ki in row k for each of its (<= 4) in-subdomain lower couplings k, 4 bits each (15: none)
  DevBuf<int> sub_int;      // subdomains none of whose rows has a partition-ghost column ...
  DevBuf<int> sub_bnd;      // ... and the others (device lists; null on a single rank)
  DevBuf<int> sub_order;    // launch order of all subdomains when they differ in cost (ragged bricks): inside each XCD's
                            // contiguous eighth the long ones first, so the short ones make the tail; null: uniform
  DevBuf<int> row_uoffw;      // first parked upper block of a row inside its subdomain, all (<= 4) uppers counted
  // Brick-local 16-bit column indices for k_pc_park (2 x 2 blocks): entry = segment << 13 | offset, column = the brick's
  // sub_seg[segment] + offset.  Segment 0 starts at the brick's own first row; the others cover what its rows reach in
  // other bricks and among the ghost columns, windows of 8192 columns each (a 16 x 16 x 2 brick of a structured mesh:
  // its six neighbour bricks).  Null when some brick would need more than 8 segments: the int32 planes serve then.
  DevBuf<unsigned short> col16;      // [n][8]: the (<= 8) slots of a row together, 16 bytes -- one load per row instead of one per slot
  DevBuf<int> sub_seg;               // [nsub][8]
  // With the indices brick-local, everything a row's descriptors say -- row_info, row_uoff, its col16 record: 24 bytes -- is
  // brick-local, and bricks of the same shape and surroundings have the same descriptors byte for byte (216^3 in 16 x 16 x 2
  // bricks: 13 x 13 x 108 of the 14 x 14 x 108 are full interior bricks).  k_pc_park on col16 reads ONE copy of each
  // distinct table (a template: rows [sub_desc[s], sub_desc[s] + rows of brick s) of t_*), small enough to stay in L2,
  // instead of streaming every brick's own from HBM.  A mesh without repeats gets one template per brick.
  // WAI_NO_DESC_SHARE (read_env): the same kernel on the per-row arrays, sub_desc = sub_ptr.
  DevBuf<int> t_info, t_uoff;        // [template rows]
  DevBuf<unsigned short> t_col16;    // [template rows][8]
  DevBuf<int> sub_desc;              // [nsub]: first row of the brick's template
  // short bricks packed into shared k_pc_park workgroups (ilu_schedule.hpp, phase 10): per launch list -- 0 all subdomains,
  // 1 sub_int, 2 sub_bnd -- the (group, wave) records [n_groups][8][4], or null where nothing packs
  DevBuf<int> pack_tab[3];
  DevBuf<int> ord_f;          // big, wide: rows sorted by forward level, ...
  DevBuf<int> ord_b;          // ... by backward level (row ranges of each level: lev_f_ptr / lev_b_ptr)
  // big, not sublu, tiles set: the substitution sweeps run one launch per TILE level where tiles.serve (launch_big_solve)
  TileTables tiles;
  // wai_ctx::ilu only: the system whose preconditioner is set up now (null: none) -- the factor buffers above are shared by
  // the flow and the scalar tracer systems, and one record serves the extended systems' and the coupled system's own
  // buffers too.  Set by do_pc_setup; pc_invalidate when a system's values or the preconditioner's kind change
  const LinSys* owner = nullptr;
};
// Block-Jacobi ILU(0) in multicolour order (wai_set_pc_ordering; colour_order.hpp, where build_colour_order makes the facts
// and every table on the host): the tables on the device.  The flow system's alone; the factor itself goes to the shared
// buffers of wai_ctx::ilu (fval: L multipliers, U and, in the diagonal slot, the inverted pivot; dinv), one system's factor at
// a time as ever (IluSchedule::owner).  built: the tables stand for the subdomains and the pattern in force
struct ColourSchedule : ColourFacts {
  bool built = false;
  bool fused = false;       // k_pc_colour serves (pc_colour_serves, recorded by the set-up): diag_only, rows of <= 8 blocks, subdomains that fit a
                            // workgroup (1024 rows at block sizes 1 and 2, 512 at 3, 256 at 4), one rank, WAI_COLOUR_SWEEPS unset
  DevBuf<int> sub_ptr;      // [nsub + 1] row ranges
  DevBuf<int> sub_ncol;     // [nsub] colours of the subdomain
  DevBuf<int> rows;         // the launch lists: all rows sorted by (colour, row); colour c is rows [col_ptr[c], col_ptr[c + 1])
  DevBuf<unsigned long long> slots;   // per row: its in-subdomain slots in elimination order, 4 bits each, lower ones first
  DevBuf<int> counts;       // per row: lower | upper << 8 | diagonal slot << 16 | colour << 24
};
// The coarse level of the two-level preconditioner (wai_set_pc_coarse; coarse_space.hpp, where build_coarse_space makes every
// list on the host): the lists on the device, the dense Galerkin matrix and its inverse, and the work vectors of an
// application.  The flow system's alone.  mode: WAI_PC_COARSE_OFF | _ADDITIVE | _DEFLATED; the lists stand from the call
// that set them, Ac and Ainv from the set-up in force (IluSchedule::owner)
struct CoarseLevel {
  int mode = 0;
  CoarseSpace h;            // what the device's lists were made from
  int m = 0, nblk = 0;      // coarse unknowns nc * bs, blocks of the coarse pattern
  DevBuf<int> agg, agg_ptr, agg_rows;                       // [n], [nc + 1], [n]
  DevBuf<int> blk_row, blk_col, ent_ptr, ent_row, ent_slot; // per coarse block: its place in Ac and its contribution list
  DevBuf<double> Ac, W, Ainv;                               // [m][m] row-major: Galerkin matrix, elimination workspace, inverse
  DevBuf<double> prow, pcol;                                // [m] the elimination's scaled pivot row and pivot column
  DevBuf<int> perm, src;                                    // [m] row exchanges of the elimination; columns of W that make Ainv
  DevBuf<double> rc, yc;                                    // [m] restricted residual, coarse correction
  DevBuf<double> t, w;                                      // deflated mode: P yc (halo room) and A P yc, then r - A P yc
  float ms_galerkin = 0.f, ms_inverse = 0.f;                // the last set-up's two parts, timed while profiling is on
};
// threads of a brick kernel's workgroup: one per row of the largest subdomain, whole waves
inline int pc_threads(const IluSchedule& s) { return ((s.max_rows + 63) / 64) * 64; }

// A run-time block size or flag turned into a template argument, once: f(std::integral_constant<int, BS>{}) for bs 1 .. 4
// (else -1, f not called) and f(std::true_type{} / std::false_type{}).  Inside f: `constexpr int BS = decltype(bs)::value;`
template <class F>
int with_bs(int bs, F&& f) {
  switch (bs) {
    case 1: f(std::integral_constant<int, 1>{}); return 0;
    case 2: f(std::integral_constant<int, 2>{}); return 0;
    case 3: f(std::integral_constant<int, 3>{}); return 0;
    case 4: f(std::integral_constant<int, 4>{}); return 0;
    default: return -1;
  }
}
template <class F>
void with_flag(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}
// The run-time equation of state likewise: f(std::integral_constant<int, EOS_...>{}) for the seven kinds (else -1, f not
// called; wai_ctx_create refuses such a kind).  Inside f: `constexpr int K = decltype(k)::value;`
template <class F>
int with_eos(int kind, F&& f) {
  switch (kind) {
    case EOS_W: f(std::integral_constant<int, EOS_W>{}); return 0;
    case EOS_WE: f(std::integral_constant<int, EOS_WE>{}); return 0;
    case EOS_WCE: f(std::integral_constant<int, EOS_WCE>{}); return 0;
    case EOS_WSE: f(std::integral_constant<int, EOS_WSE>{}); return 0;
    case EOS_WAE: f(std::integral_constant<int, EOS_WAE>{}); return 0;
    case EOS_WSCE: f(std::integral_constant<int, EOS_WSCE>{}); return 0;
    case EOS_WSAE: f(std::integral_constant<int, EOS_WSAE>{}); return 0;
    default: return -1;
  }
}
// what the host asks of an EOS, from EosT<K> / is_salt<K>; -1 for an unknown kind (t untouched)
struct EosTraits { int np, df, nmob; bool salt; };
inline int eos_traits(int kind, EosTraits& t) {
  return with_eos(kind, [&](auto k) {
    constexpr int K = decltype(k)::value;
    t = EosTraits{EosT<K>::np, EosT<K>::df, EosT<K>::nmob, is_salt<K>};
  });
}

// PCASM (restricted additive Schwarz) system: every subdomain's overlapped row set is stored as
// its own block of an extended matrix E (couplings leaving the set dropped), so the block-Jacobi
// machinery applies to E unchanged: gather r -> r_ext, ILU(0) solve per block, scatter the owned
// rows back (src/timestepper.F90:1668-1669,1753-1757; PETSc PCASM defaults: overlap 1, restrict).  Where every block of E
// fits one workgroup the gather, the sweeps, the scatter and the SpMV before them are ONE launch instead (`fused` below)
struct AsmSystem {
  int overlap = -1;           // what E was built for (-1: not built; 0: no overlap, fill only)
  int levels = 0;             // ILU(k) fill levels E's pattern carries
  bool sublu = false;         // ... or the complete fill of sub-preconditioner lu (levels is 0 then)
  // block-Jacobi ILU(k), k > 0, in one fused launch: no overlap, so E's rows are the system's own rows in their order and
  // E's pattern is the factor's (the Jacobian's in-brick blocks + fill, <= 16 per row); `sched` is wide and k_pc_wide's
  // two-pattern form multiplies by A on the Jacobian's planes and sweeps the factor on E's (fuse_asked: what the set-up
  // asked for -- the schedule may still have said no: fill wider than 16 blocks, a subdomain of more than 1024 rows)
  // PCASM in one fused launch (overlap > 0, ILU(k), k >= 0): E's rows are the overlapped blocks' (n_ext > N), the same
  // two-pattern form reads the operator through ext_row (k_pc_wide<.., MAP>: host.hpp, pc_asm_fused) and writes the rows a
  // block owns.  Same two flags: asked for on the flow system, one rank, a mesh of <= 8 blocks per row, no network blocks,
  // no sub lu, WAI_ASM_UNFUSED unset; refused by the schedule where an extended block has more than 1024 rows (a
  // 16 x 16 x 2 brick at overlap 1: 1152) or a row of E more than 16 blocks
  bool fused = false, fuse_asked = false;
  int n_ext = 0;
  Bcsr E;                     // block-ELL over the n_ext rows, columns in ext numbering: a view of ...
  DevBuf<int> E_col;          // ... its column planes and
  DevBuf<double> E_val;       // ... its values, owned here
  IluSchedule sched;
  DevBuf<int> ext_row;        // [n_ext] row of the global system, bit 31 set: owned by this block
  DevBuf<int> gmap;           // [W * n_ext] plane position (slot * n + row) of the source block in J, -1: none
  DevBuf<double> r_ext;       // [bs * n_ext] gathered right-hand side / solution
  // overlap across rank boundaries: the matrix rows of the partition-ghost cells, received from
  // their owners at every set-up (block-ELL over the n_halo cells, the sender's slot order), and the residual
  // with its ghost entries filled by one more halo exchange per application
  // the source network's blocks inside the factor's pattern (src/flow_simulation.F90:3023-3084 widens the BAIJ pattern
  // PETSc factors): E's pattern carries the pairs of network cells of one subdomain, net_pos / net_pair name where each
  // block of the network's E goes (plane position t * n_ext + q; pair = row * m + column in the coupling array)
  bool with_net = false;
  int n_net = 0;
  DevBuf<int> net_pos;
  DevBuf<int> net_pair;
  bool cross = false;
  DevBuf<double> hval;        // [W * bs * bs * n_halo]
  DevBuf<double> r_full;      // [bs * n_prim]
};

// Residual form of the time stepping method (src/timestepper.F90:345-452), by value to kernels
struct ResForm {
  int method = 0;             // WAI_METHOD_BEULER | BDF2 | DIRECTSS
  double dt = 0.0, ratio = 0.0;
  const double* last = nullptr;   // lhs at the start of the step
  const double* last2 = nullptr;  // BDF2: lhs one step further back
};

// Passive tracers (src/tracer.F90:30-40).  Their two linear systems -- one scalar system at a time, or all nt coupled -- are
// wai_ctx::aux and wai_ctx::coupled (LinSys below), which hold the values, the solver settings and the work vectors.
constexpr int MAX_TRACERS = 8;
constexpr int POST_OFF = 64;   // h_scal[POST_OFF ..+2]: {(R,R), 8 * sequence number + code, check word} posted by the device (post_scalars)
constexpr unsigned long long POST_KEY = 0x5bd1e995a5a5c3c3ull;   // check = bits((R,R)) ^ bits(tag) ^ POST_KEY: zeroed memory never verifies
struct Tracers {
  int nt = 0;
  int phase[MAX_TRACERS] = {0};
  double decay[MAX_TRACERS] = {0}, activation[MAX_TRACERS] = {0}, diffusion[MAX_TRACERS] = {0};
  // views: the struct is a kernel argument, so the owners live beside it in the context (wai_ctx::tr_bc, tr_inj, tr_rhsb)
  double* bc = nullptr;    // [n_bc][nt] Dirichlet mass fractions
  double* inj = nullptr;   // [n_sources][nt] injection rates
  double* rhsb = nullptr;  // coupled mode: [n_prim * nt + 16] right-hand side, interleaved [cell][nt] (allocated on first use)
  int mode = 0;            // WAI_TRACER_PER_TRACER | WAI_TRACER_COUPLED (wai_set_tracer_solve_mode)
  long long n_sweeps = 0;  // assembly sweeps over the faces so far (wai_tracer_stats)
  // k_tracer_assemble_all and k_tracer_lhs take this struct BY VALUE: its size fixes where their later arguments sit.  The
  // solver state that used to follow (now in LinSys) leaves this tail, so that both kernels keep their argument layout --
  // dropping it is a change of device code and belongs with one
  unsigned char kernarg_tail[136] = {0};
};
static_assert(sizeof(Tracers) == 408, "Tracers is a kernel argument (k_tracer_assemble_all, k_tracer_lhs): its size is part of their argument layout");
static_assert(std::is_trivially_copyable<Tracers>::value, "a kernel argument holds views, never an owner");

// one tracer's system: which tracer, and the method's combination (timestepper.F90:458-581)
struct TracerForm {
  int method, it, nt, phase;
  double dt, ratio, decay, activation, diffusion;
};
static_assert(std::is_trivially_copyable<TracerForm>::value && std::is_trivially_copyable<ResForm>::value &&
              std::is_trivially_copyable<EosParams>::value, "a kernel argument holds views, never an owner");

// Finalisation of a producer kernel's partial sums inside its own launch (fin_block, reductions.hip.h): one
// extra workgroup waits for the partials of `nslots` consecutive reduction slots, sums them into the device
// scalars -- in the order k_finalize sums them --, derives the BiCGStab scalars of `phase` and, when asked,
// posts the scalars to the pinned host mirror.  Replaces a one-block k_finalize launch (and the 128-byte
// copy) behind every producer.
constexpr int FIN_MAXF = 64;   // most finaliser workgroups of a launch (second-level partials per slot)
struct Fin {
  int count = 0;               // workgroups of this launch that store partials; 0: no finalisation here (no extra workgroup)
  int nb = 0;                  // partials per slot to sum (an earlier launch may have left some of them)
  int nf = 1;                  // finaliser workgroups: the last nf of the grid, each sums one slice of the partials (fin_slices)
  double* part2 = nullptr;     // [slots][FIN_MAXF] slice sums on their way to the last finaliser
  int slot0 = 0, nslots = 0;
  int phase = -1;              // derive_scalars phase, -1: sums only
  int seq = 0;                 // > 0: post (R,R) and the breakdown code with this sequence number to `post`
  double* scal = nullptr;
  double* post = nullptr;      // device address of the pinned host mirror (16 bytes, 16-byte aligned)
};
static_assert(std::is_trivially_copyable<Fin>::value, "a kernel argument holds views, never an owner");

// The reduction workspace of the Krylov helpers: device scalars, partial sums, the posted scalars' mirror and the launch
// counters.  Single and shared: one solve runs at a time on the library's stream, whichever system it solves.
struct Krylov {
  double* d_post = nullptr;    // device address of h_scal + POST_OFF (a view)
  int seq = 0;                 // last sequence number handed out
  long long n_launch = 0, n_copy = 0;   // kernels launched / copies enqueued by the Krylov helpers (wai_launch_stats)
  DevBuf<double> partials;     // [slots][nb_max]
  DevBuf<double> partials2;    // [slots][FIN_MAXF]: slice sums of the finaliser workgroups (fin_block)
  DevBuf<unsigned> started;    // k_bcgs_xrp<DERIVE>: workgroups of the launch that have read their scalars (device counter, zero between launches)
  bool alpha_pending = false;  // several ranks: alpha = rho / (V,rP) is to be derived by the next pack_halo_axpy launch (no scalar kernel)
  int nb_max = 0;
  DevBuf<double> scal;         // device scalars
  PinnedBuf<double> h_scal;    // pinned host mirror
  int nblocks = 0;
  int nb_pc = 0;               // partial-sum blocks the last preconditioner application left per slot
};

// A set of Krylov work vectors
struct KrylovVecs {
  DevBuf<double> R, RP, P, V, S, T, tmp, X_own;   // nl + 16 doubles each (alloc_krylov_vecs)
  double* X = nullptr;         // BiCGStab's iterate, a view: the caller's x during a solve (ksp_bcgs), X_own otherwise
  DevBuf<double> bl;           // BiCGStab(L): r_0..r_L, u_0..u_L, r~ (allocated on first use)
  DevBuf<double> basis;        // GMRES: (basis_m + 4) vectors of nl (ensure_basis)
  int basis_m = 0;
};

struct KspOpts {
  int type = WAI_KSP_BCGS, restart = 30, max_its = 10000;
  double rtol = 1.e-5, atol = 1.e-50;
};
// A system's preconditioner: kind, PCASM overlap, ILU(k) levels, sub-preconditioner.  type = WAI_AUX_PC_FOLLOW: the system has
// none of its own and takes the flow solver's (wai_ctx::opts and wai_ctx::sub_pc) -- read through pc_of (host.hpp), never
// directly
struct PcOpts {
  int type = WAI_AUX_PC_FOLLOW, asm_overlap = 1, ilu_levels = 0, sub = WAI_SUB_ILU;
};

// One linear system: everything the Krylov drivers, the preconditioner set-up and the launchers below them need to know
// about the system they work on, handed to them as an argument.  The context holds three, all on the mesh's pattern:
//   flow     the flow Jacobian, block size np; built in wai_ctx_create
//   aux      one scalar tracer system at a time, block size 1; built in wai_set_tracers.  Its kv ALIASES the flow's work
//            vectors and GMRES basis (it uses the first n_prim entries of each vector, basis vectors n_prim apart; the two
//            never solve at once).  So a per-tracer GMRES restart is clamped to the flow's basis size: the
//            min(restart, basis_m) in ksp_gmres sees the flow's basis_m
//   coupled  all nt tracer systems as one (Bcsr::dg), vectors of nt * n_prim; values, factor, vectors and basis its own
//            (wai_ctx::kv_coupled), allocated on first use
// Each system has its preconditioner's settings too (pc; pc_of in host.hpp): the flow's follow wai_ctx::opts and
// wai_ctx::sub_pc, and so do the two tracer systems' until wai_set_aux_pc gives them their own.
// Single and shared, NOT part of a system: the pattern (wai_ctx::pat), the subdomain list and the ILU schedule on it with
// its factor buffers (wai_ctx::ilu: it depends on the pattern alone; one system's factor at a time, IluSchedule::owner), the
// dense block inverses of preconditioner lu (wai_ctx::lu, likewise) and the reduction workspace (wai_ctx::ks).
struct LinSys {
  Bcsr A;               // the values on the shared pattern; A.bs: unknowns per cell = block size = dof of the halo exchange
  DevBuf<double> val, fdg;   // what A.val and A.fdg point to, owned here
  KspOpts ksp;
  PcOpts pc;            // its preconditioner, or "the flow solver's" (the flow system's always is)
  int n = 0, nl = 0;    // A.bs * n_owned, A.bs * n_prim
  KrylovVecs* kv = nullptr;   // wai_ctx::kv (flow, aux) or wai_ctx::kv_coupled (a view)
  AsmSystem as;         // its extended system (PCASM, ILU(k), network blocks in the factor), built on first use
  bool net_blocks = false;   // the source network's coupling blocks E belong to its operator (the flow system only)
};

// Gather of output rows to one rank (wai_gather_rows, wai_gather_fluid; gather.hip).  Every buffer is sized on first use,
// grown when a call needs more and kept: a run's snapshots ask for the same sizes every time.
struct Gather {
  DevBuf<double> in;      // a host `local` staged
  DevBuf<double> send;    // [rows][ncomp + 1]: the packed rows, each followed by its place as a double
  DevBuf<double> recv;    // root: every rank's slab, in rank order
  DevBuf<double> out;     // root: a host `out` staged
  DevBuf<double> counts;  // [nranks] row counts, all-reduced
  DevBuf<int> idx;        // a host `index` staged
  DevBuf<int> claim;      // root: [n_global] received row that took the place, -1: free
  DevBuf<int> flag;       // root: [4] error code (0 none, 1 place out of range, 2 place claimed twice), place, the two received rows
  size_t n_in = 0, n_send = 0, n_recv = 0, n_out = 0, n_counts = 0, n_idx = 0, n_claim = 0;   // elements each buffer holds
};

}  // namespace wai

namespace wai {
// PCLU / sub-preconditioner "lu" (src/timestepper.F90:1749-1750; the reference lists it "for testing
// purposes"): exact solves of the preconditioner blocks.  Each block's dense inverse, formed on the
// host with partial pivoting at every set-up, applied on the device as one dense product per block.
struct LuBlocks {
  DevBuf<double> inv;         // concatenated dense inverses, block b at inv_ptr[b], row-major m_b x m_b
  DevBuf<size_t> inv_ptr;     // device, nsub + 1
  std::vector<size_t> h_inv_ptr;
  size_t total = 0;
  int bs = 0;                 // block size the offsets were laid out for (the flow's and the tracers' differ)
};
int launch_lu_apply(wai_ctx* c, int bs, const double* r, double* z);

// The streams, the events and the communicator of a context.  A base of wai_ctx, so that its destructor runs after the
// members' -- every device buffer is released first, then the events and streams, then the communicator (context.hip)
struct Handles {
  hipStream_t stream = nullptr;
  Comm* comm = nullptr;
  hipEvent_t ev_scal = nullptr;   // marks the scalar read-back of a Krylov iteration (ksp_bcgs)
  // halo exchange overlapped with the preconditioned operator on the bricks that touch no ghost
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_pack = nullptr, ev_halo = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, pev0 = nullptr, pev1 = nullptr;   // measurement
  Handles() = default;
  Handles(const Handles&) = delete;
  ~Handles();
};
}  // namespace wai

// Every DevBuf below, and in the structs below, is released when the context is deleted (wai_ctx_destroy): a new buffer is
// a new field and nothing else
struct wai_ctx : wai::Handles {
  int device = 0;
  int n_cu = 256;               // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  size_t lds_per_block = 64 * 1024;   // LDS a workgroup may ask for (hipDeviceAttributeMaxSharedMemoryPerBlock; 160 KB on gfx950)
  int kind = 0, np = 0, df = 0, nmob = 0;   // the EOS, and its EosTraits (wai_ctx_create)
  bool salt = false;
  wai::EosParams ep{};
  wai_solver_opts opts{};
  int sub_pc = WAI_SUB_ILU;     // sub-preconditioner of bjacobi / asm (wai_set_sub_pc): ILU(ilu_levels) or the blocks' exact LU
  int net_pass = WAI_NETWORK_PASS_HOST;     // wai_set_network_pass: where the source network's pass runs (net_on_device: what is in force)
  int net_walk = WAI_NETWORK_WALK_LANE;     // wai_set_network_walk: how the device pass walks groups and reinjectors (net_walk_wave: what is in force)
  int net_wave_attr = 0;                    // the wave kernels that were allowed their dynamic LDS above 64 KB (bit 0 k_network_pass_wave, 1 k_cb_pass_wave)
  long long net_passes = 0, net_waits = 0;  // passes made / stream waits issued by network_update and network_couplings (wai_test_network_stats)
  int cp_build = WAI_COUPLING_BUILD_COLUMNS;   // wai_set_coupling_build: how the network's Jacobian blocks are built (cp_batched: what is in force)
  long long cp_launches = 0, cp_columns = 0, cp_chunks = 0;   // kernel launches, columns and chunks of the last coupling build (wai_test_coupling_build_stats)
  int pc_ordering = WAI_PC_ORDER_NATURAL;   // wai_set_pc_ordering: elimination order of the flow system's block-Jacobi ILU(0)
  wai::ColourSchedule colour;   // ... its symbolic phase under WAI_PC_ORDER_MULTICOLOUR, built by the first set-up that needs it
  wai::CoarseLevel coarse;      // wai_set_pc_coarse: the flow system's coarse level (pc_coarse: is it in force)
  std::vector<int> pc_tiles;    // wai_set_pc_tiles: row ranges [n_tiles + 1] of the tiles that refine the subdomains; empty: none
  wai::DeviceMesh mesh;
  wai::Sources src;
  wai::Network net;
  std::vector<int> src_gidx;    // wai_set_source_global_index: global index of every local source (networks across ranks)
  int src_nglobal = 0;
  wai::Pattern pat;
  wai::LinSys flow, aux, coupled;
  wai::KrylovVecs kv, kv_coupled;
  wai::IluSchedule ilu;
  wai::LuBlocks lu;
  wai::Krylov ks;
  wai::Tracers tr;
  wai::Gather gat;
  wai::DevBuf<double> tr_bc, tr_inj, tr_rhsb;   // what tr.bc, tr.inj and tr.rhsb point to (Tracers is a kernel argument: views only)
  // fluid state, SoA df x n_local each; perturbed states np x df x n_prim
  wai::DevBuf<double> flu, flu_last_iter, flu_last_step, flu_pert;
  wai::DevBuf<double> hstep;    // FD steps np x n_prim (interleaved like y)
  // work vectors (interleaved [cell][bs], nl entries)
  wai::DevBuf<double> w_y, w_yold, w_delta, w_f, w_lhs, w_a, w_b, w_c;
  wai::DevBuf<int> d_flags;     // [0] err, [1] first bad cell, [2] changed_y, [3] changed_search
  wai::PinnedBuf<int> h_flags;
  wai::DevBuf<double> d_red;    // reduction scratch
  wai::PinnedBuf<double> h_red;
  wai::DevBuf<double> stage[4]; // host-vector staging
  size_t stage_len = 0;
  // run-time switches of the fused launches, read from the environment once per solve / set-up / probe (read_env),
  // not per launch: WAI_FIN_SEPARATE, WAI_NO_COL16 (k_pc_park on the int32 column planes), WAI_BCGS_SCALAR_KERNELS
  // WAI_ILUK_LEVEL_PATH: block-Jacobi ILU(k) keeps the launch-per-level path where the fused launch would serve (tests
  // that compare the two paths in one process; read at the preconditioner's set-up); WAI_ASM_UNFUSED: PCASM likewise keeps
  // its launches (k_spmv, gather, the sweeps on the extended system, scatter, the reductions) where the fused one would serve;
  // WAI_NO_DESC_SHARE: k_pc_park on col16 reads every brick's own descriptors instead of the shared templates
  // WAI_NO_PACK: one k_pc_park workgroup per brick on a schedule that has packed groups (the A/B and the bit-identity tests)
  // WAI_PARK_STAGE=0|1: k_pc_park's operator launches without / with the brick's operand segment staged in LDS
  // WAI_COLOUR_SWEEPS: the multicolour ordering keeps its launch-per-colour path (k_colour_sweep) where the fused launch
  // k_pc_colour would serve (the tests' comparison and the timing tool; read at the preconditioner's set-up)
  struct EnvSw {
    bool fin_separate = false; bool no_col16 = false; bool scalar_kernels = false; bool iluk_level_path = false;
    bool asm_unfused = false; bool no_desc_share = false; bool no_pack = false;
    bool colour_sweeps = false;
    bool pc_unfused = false;   // WAI_PC_UNFUSED: pc_amul takes its unfused route (t = A x, then pc_solve) where a fused launch would serve -- the
                               // route a coarse level puts the flow system on, without one (tools/pc_coarse_timing.py)
    int park_stage = -1;   // WAI_PARK_STAGE: 0 / 1 k_pc_park's staged operand off / on for every launch kind, -1 the compiled-in defaults
  } env;
  int test_drop_wait = 0;   // fault injection (wai_test_drop_stream_wait): 1 the face bricks' launch does not wait for the halo
  // halo
  int n_nbr = 0;
  std::vector<int> nbr_rank, send_ptr, recv_ptr;
  wai::DevBuf<int> d_send_idx; wai::DevBuf<double> d_sendbuf, d_recvbuf;
  int send_total = 0, max_dof_buf = 0;
  // Newton bookkeeping
  double fnorm0 = 0.0;
  // time stepping method: residual form in force, and wai_timestep's own BDF2 history
  int method = 0;               // residual form (wai_set_residual_form)
  double ratio = 0.0;
  wai::DevBuf<double> w_lhs2;   // lhs two steps back, as handed to wai_set_residual_form
  int scheme = 0, taken = 0;    // wai_set_timestep_method, accepted wai_timestep calls since
  double dt_last = 0.0;
  wai::DevBuf<double> w_hist;   // lhs at the start of the last accepted wai_timestep
  wai::DevBuf<double> w_hist_prev;  // ... and of the one before, to undo an acceptance
  double dt_last_prev = 0.0;
  bool can_reject = false;      // the last wai_timestep converged and has not been rejected
  // measurement
  bool prof_on = false;
  bool last_iter_partial = false;   // flu_last_iter holds only the transition sweep's planes (do_newton_step)
  double prof_ms[wai::KC_COUNT] = {0};
  long long prof_n[wai::KC_COUNT] = {0};
  std::string err;
  bool bc_set = false;
  int dbg = 0;                  // timing probes (wai_bench_kernel)
};

// ---- kernel launchers (kernels_eos.hip, kernels_residual.hip, kernels_jacobian.hip, kernels_tracer.hip / kernels_matrix.hip, kernels_factor.hip, kernels_fused.hip) ----
namespace wai {
int launch_eos(wai_ctx* c, const double* y, int first, int count, bool perturbed);
int launch_residual(wai_ctx* c, double dt, const double* lhs_old, double* f, double* lhs_out,
                    double* rhs_out, const int* only = nullptr, int n_only = 0);   // only: these rows alone (device list)
int launch_jacobian(wai_ctx* c, double dt, const double* lhs_old);
int launch_transitions(wai_ctx* c, const double* y_old, double* search, double* y);
// tracer system of tf.it on the mesh's pattern: values -> c->aux.A.val, rhs -> b
int launch_tracer_assemble(wai_ctx* c, const TracerForm& tf, const double* alx_last,
                           const double* alx_last2, double* b);
// all nt systems in one sweep over the faces: values -> c->coupled.A.val ([slot][tracer][row]), rhs -> b ([row][tracer])
int launch_tracer_assemble_all(wai_ctx* c, int method, double dt, double ratio, const double* alx_last,
                               const double* alx_last2, double* b);
int launch_tracer_lhs(wai_ctx* c, double* Al);
int launch_separator(wai_ctx* c, double pressure, double* out);   // out[3] on the device: hf, hg, err
int launch_face_fluxes(wai_ctx* c, const int* face_cells, double* out);   // [face][np + nmob]
int launch_source_rates(wai_ctx* c, double* out, bool raw = false);
// kernels_network.hip: one pass of the network on the device (raw: launch_source_rates(c, raw, true)), and the coupling
// build's column steps
int launch_network_pass(wai_ctx* c, const double* raw, double* net, double* enth, double* state_out, bool wave);
int net_wave_allow_lds(wai_ctx* c, const void* kernel, int bit, size_t* bytes);
int launch_cp_perturb(wai_ctx* c, double* p, double* yh);
int launch_cp_restore(wai_ctx* c, double* p, const double* yh);
int launch_cp_diff(wai_ctx* c, int ml, int m, int bs, int j, int k, const double* g, const double* yh, double* val, int* flag);   // out[0..n) rates, out[n..2n) enthalpies (device); raw: before the network pass
// kernels_coupling.hip: the columns col0 .. col0 + ncol - 1 of the batched coupling build on the scratch plan b -- five
// launches whatever ncol is; launches: counted
int launch_coupling_batch(wai_ctx* c, const CouplingBatch& b, int col0, int ncol, double dt, const double* y, const double* lhs_old,
                          long long* launches, bool wave);
// X[cell][nt] <-> x[cell] of tracer it; alx = Al o X
int launch_tracer_pick(wai_ctx* c, const double* X, int it, double* x);
int launch_tracer_put(wai_ctx* c, const double* x, int it, double* X);
int launch_tracer_alx(wai_ctx* c, const double* X, double* alx);
int launch_max_scaled(wai_ctx* c, const double* v, const double* scale, double tol, double* val,
                      int* idx);
int launch_fluid_aos(wai_ctx* c, const double* flu_soa, double* out_aos);
int launch_region_get(wai_ctx* c, double* out);  // regions as doubles, n_prim
int launch_region_set(wai_ctx* c, const double* in, int first, int count);

int launch_spmv(wai_ctx* c, const Bcsr& M, const double* x, double* y);
// ILU(0) of any (matrix, schedule) pair: a system's matrix with the brick schedule, or its extended ASM system with its own
int launch_ilu_factor_on(wai_ctx* c, const Bcsr& M, IluSchedule& s);
// in2 (optional, fused kernels that can: pc_axpy_capable): the input is in - alpha in2, alpha = the device scalar S_ALPHA
// F (optional, wide schedules): the factor has a pattern of its own (ILU(k) fill: AsmSystem::E of a fused system) -- M is
// the operator A, read on its own planes, `s` the schedule of F, whose column planes the sweeps follow
// row_map (optional, with F): F's rows are not M's -- PCASM's extended system; AsmSystem::ext_row maps each to its row of M
// and marks the rows its block owns, the only ones written (k_pc_wide<.., MAP>); z != in
int launch_pc_on(wai_ctx* c, const Bcsr& M, const IluSchedule& s, bool spmv, const double* in, double* z,
                 int dot_mode, const double* aux, const int* list = nullptr, int nrun = 0, const Fin* fin = nullptr,
                 const double* in2 = nullptr, const Bcsr* F = nullptr, const int* row_map = nullptr);
// which fused kernel serves (matrix, schedule): 4 k_pc_wide, 3 k_pc_wave, 2 k_pc_rows, 1 k_pc_park, 0 the generic k_pc,
// -1 the coupled tracer system's k_dg_pc
int pc_kernel_kind(const wai_ctx* c, const Bcsr& M, const IluSchedule& s);
bool pc_axpy_capable(const wai_ctx* c, const Bcsr& M);
bool pc_axpy_default(const wai_ctx* c, const Bcsr& M);   // is the composed second launch the default for the kernel in force (k_pc_park with col16)
// subdomains of any size: level-by-level launches, in place on z (z = r on entry)
int launch_big_solve(wai_ctx* c, const Bcsr& M, const IluSchedule& s, double* z);
// multicolour order (ColourSchedule): the factor of M into s.fval / s.dinv, one launch per colour; both substitutions in place
// on z, 2 colours - 1 launches of k_colour_sweep
int launch_colour_factor(wai_ctx* c, const Bcsr& M, const ColourSchedule& k, IluSchedule& s);
int launch_colour_solve(wai_ctx* c, const Bcsr& M, const ColourSchedule& k, const IluSchedule& s, double* z);
// the fused launch of the multicolour ordering (k_pc_colour): does it serve (the set-up records the answer in k.fused), and
// z = B^-1 (A in) or B^-1 in with launch_pc's dot modes and finalisation
bool pc_colour_serves(const wai_ctx* c, const Bcsr& M, const ColourSchedule& k, bool one_rank);
int launch_pc_colour(wai_ctx* c, const Bcsr& M, const ColourSchedule& k, const IluSchedule& s, bool spmv, const double* in, double* z,
                     int dot_mode, const double* aux, const Fin* fin = nullptr);
// the coarse level (kernels_coarse.hip): Ac from the system's value planes; Ainv from Ac (2 m + 2 launches; a zero pivot raises
// d_flags[0]); rc = P^T r; yc = Ainv rc; z += P yc (add) or z = P yc
int launch_coarse_galerkin(wai_ctx* c, const Bcsr& A, CoarseLevel& k);
int launch_coarse_invert(wai_ctx* c, CoarseLevel& k);
int launch_coarse_restrict(wai_ctx* c, const CoarseLevel& k, const double* r, double* rc);
int launch_coarse_gemv(wai_ctx* c, const CoarseLevel& k, const double* rc, double* yc);
int launch_coarse_prolong(wai_ctx* c, const CoarseLevel& k, const double* yc, double* z, bool add);
// sub-preconditioner lu (IluSchedule::sublu): both substitutions of every block in one launch, in place on z
int launch_sublu_solve(wai_ctx* c, const Bcsr& M, const IluSchedule& s, double* z);
bool sublu_vector_in_lds(const IluSchedule& s, int bs);   // does k_sublu_solve hold a block's part of the vector in LDS
int launch_asm_gather_matrix(wai_ctx* c, const Bcsr& M, const AsmSystem& a);   // a.E.val <- M.val (and the ghost cells' rows; + the network's blocks)
int launch_pack_rows(wai_ctx* c, const Bcsr& M);                              // d_sendbuf <- matrix rows of the cells sent to neighbours
int launch_unpack_rows(wai_ctx* c, const Bcsr& M, const AsmSystem& a);        // a.hval <- d_recvbuf
int launch_asm_gather(wai_ctx* c, const AsmSystem& a, const double* r);       // a.r_ext <- r
int launch_asm_scatter(wai_ctx* c, const AsmSystem& a, double* z);            // z[owned] <- a.r_ext
// up to two dot products (a1,b1) -> slot1, (a2,b2) -> slot2 (a2 null: one); partial blocks in ks.nb_pc
int vec_dots(wai_ctx* c, const double* a1, const double* b1, int slot1, const double* a2, const double* b2,
             int slot2, int n);
// z = B^-1 r (spmv = false) or z = B^-1 (A x) (spmv = true: x is `in`, haloed by the caller).
// dot_mode: the inner products reduced on the way (PcDot above), aux the partner of modes 1 and 4
// list / nrun: run only the listed subdomains (null: all)
// fin (optional): finalise the dot products in the kernel's last workgroup instead of a k_finalize launch
int launch_pc(wai_ctx* c, const Bcsr& M, bool spmv, const double* in, double* z, int dot_mode, const double* aux,
              const int* list = nullptr, int nrun = 0, const Fin* fin = nullptr, const double* in2 = nullptr);
// finalisation descriptor for slots [slot0, slot0 + nslots) (the launcher fills in the workgroup counts);
// post: mirror the scalars to the host with a fresh sequence number (left in ks.seq)
Fin make_fin(wai_ctx* c, int slot0, int nslots, int phase, bool post = false);
// the same for the slots of a dot mode (PcDot)
inline Fin make_fin_dots(wai_ctx* c, int dot_mode, int phase, bool post = false) {
  return make_fin(c, pc_dot_slot0(dot_mode), pc_dot_nslots(dot_mode), phase, post);
}
int launch_ell_to_bcsr(wai_ctx* c, const Bcsr& M, double* bcsr);   // M.val on the BCSR pattern
// the coupled tracer system (Bcsr::dg; kernels_tracer_block.hip): what launch_spmv, launch_ilu_factor_on, launch_pc_on and
// launch_big_solve hand such a matrix to, and its values as [block][tracer] on the BCSR pattern
int launch_dg_spmv(wai_ctx* c, const Bcsr& M, const double* x, double* y);
int launch_dg_factor(wai_ctx* c, const Bcsr& M, IluSchedule& s);
int launch_dg_pc(wai_ctx* c, const Bcsr& M, const IluSchedule& s, bool spmv, const double* in, double* z, const int* list, int nrun);
int launch_dg_big_solve(wai_ctx* c, const Bcsr& M, const IluSchedule& s, double* z);
int launch_dg_to_bcsr(wai_ctx* c, const Bcsr& M, double* bcsr);
int launch_bcsr_to_ell(wai_ctx* c, const double* bcsr, const Bcsr& M);   // ... and back into M.val
// reductions: partial sums live in ks.partials[slot][block]; finalize sums nb partials of
// nslots consecutive slots into ks.scal and (phase >= 0) derives the BiCGStab scalars
int vec_finalize(wai_ctx* c, int nb, int slot0, int nslots, int phase);
int vec_dot(wai_ctx* c, const double* a, const double* b, int n, int slot);
int partials_clear(wai_ctx* c, int slot0, int nslots);   // reduction slots emptied (FIN_EMPTY)
int vec_copy(wai_ctx* c, double* dst, const double* src, size_t n);
int vec_zero(wai_ctx* c, double* dst, size_t n);
int vec_waxpy(wai_ctx* c, double* w, double alpha, const double* x, const double* y, int n);
int bcgs_scalars(wai_ctx* c, int phase, bool post = false);
int bcgs_update_xrp_derive(wai_ctx* c, const KrylovVecs& k, int n);
int bcgs_post(wai_ctx* c, int seq);
void read_env(wai_ctx* c);   // the launch switches above (kernels_fused.hip)
int test_drop_partials(wai_ctx* c, int n);   // fault injection (tests): workgroup 0 loses its next n partial sums
// the BiCGStab vector updates on the work vectors k, n entries each
int bcgs_update_p(wai_ctx* c, const KrylovVecs& k, int n);
int bcgs_update_s(wai_ctx* c, const KrylovVecs& k, int n);
// dots: reduces (R,R), (R,RP) into S_DP2, S_RHONEW and (fin_phase >= -1) finalises them in its last workgroup
int bcgs_update_xr(wai_ctx* c, const KrylovVecs& k, int n, bool dots = true, int fin_phase = -2, bool post = false);
// S = R - alpha V re-formed; X += alpha P + omega S; R = S - omega T; P = R + beta (P - omega V): one pass, no reduction
int bcgs_update_xrp(wai_ctx* c, const KrylovVecs& k, int n);
int pack_halo_axpy(wai_ctx* c, const double* a, const double* b, int dof, hipStream_t stream = nullptr);
// GMRES on the basis vectors v_i = basis + i * ld, n entries each
int gmres_mdot(wai_ctx* c, const double* basis, size_t ld, int n, const double* w, int k);          // scal[16+i] = (w, v_i), i<k
int gmres_maxpy_norm(wai_ctx* c, const double* basis, size_t ld, int n, double* w, int k);          // w -= sum h_i v_i ; scal[8] = |w|^2
int gmres_scale_to(wai_ctx* c, double* dst, const double* src, int slot_norm2, int n);
int gmres_update_x(wai_ctx* c, const double* basis, size_t ld, int n, double* x, const double* ycoef_host, int k);
int pack_halo(wai_ctx* c, const double* vec, int dof, hipStream_t stream = nullptr);
int unpack_halo(wai_ctx* c, double* vec, int dof, hipStream_t stream = nullptr);
}  // namespace wai
