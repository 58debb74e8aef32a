// What the cell/face assembly sweeps for gfx950 share: constants, the XCD-aware cell mapping, the mesh view, the face and
// source terms of one row, the residual forms, the records parked in LDS, and the host helpers every launcher starts from.
// Included by the five assembly units (waiwera_amd/build.py: ASSEMBLY_UNITS, all built without FMA contraction) and by
// nothing else:
//   kernels_eos.hip       k_eos / k_eos_pert (K1), k_transitions (K11), k_separator
//   kernels_residual.hip  k_residual_tile -- the default full sweep, the workgroup's own cells staged in LDS -- and
//                         k_residual (row lists; WAI_RES_TILE=0; tiles that do not fit the LDS) (K2-K4); the source-rate
//                         and face-flux outputs; the scaled max-norm (K10); the layout copies
//   kernels_jacobian.hip  k_jacobian_sym -- the default: column-wise off-diagonal blocks, own-perturbed states parked in
//                         LDS -- and the row-wise k_jacobian_park / k_jacobian (WAI_JAC_SYM=0, WAI_JAC_PARK=0) that the
//                         tests compare it with (K5)
//   kernels_tracer.hip    the tracers' scalar systems, one per tracer or all in one sweep, and their copies
//   kernels_coupling.hip  the batched build of the source network's coupling blocks: k_eos, k_source_rates and k_residual's
//                         row list per column on private scratch, around k_network_pass per column
//
// Reference loops replaced (the reference's src/):
//   flow_simulation.F90:2291-2415 fluid_properties     -> k_eos / k_eos_pert
//   flow_simulation.F90:1242-1330 cell_balances,
//   flow_simulation.F90:1334-1485 cell_inflows,
//   timestepper.F90:345-374 backwards_Euler_residual   -> k_residual_tile / k_residual (one fused sweep)
//   timestepper.F90:1584-1611 MatFDColoring + flow_simulation.F90:1102-1137 update masks
//                                                      -> k_jacobian_sym (differencing per cell: no colouring, no
//                                                         update_cell vector; every block stored by exactly one thread)
//   flow_simulation.F90:2419-2576 fluid_transitions    -> k_transitions
//   flow_simulation.F90:1489-1959 aux_lhs, aux_rhs, aux_pre_solve -> k_tracer_assemble / k_tracer_assemble_all
//   dm_utils.F90:644-685 vec_max_pointwise_abs_scale   -> k_max_scaled
//
// All kernels are HBM-bound fp64 streaming sweeps: one thread per cell, struct-of-arrays
// state so every wave instruction reads 64 consecutive doubles, neighbour gathers served by
// LDS where the default kernels hold the neighbour's record there and by L2 otherwise (brick-major numbering keeps a
// cell's 6 neighbours within a few KB).  Roofline and algorithmic bytes per cell: DESIGN.md section 4.
#pragma once
#include "context.hpp"

namespace wai {

constexpr int MAXDEG = 8;   // faces per cell held in registers (structured: 6, MINC: 7)
constexpr int MAXDEG_WIDE = MAX_CELL_FACES;   // k_tracer_assemble<K, MAXDEG_WIDE>: cells with 9 .. 16 faces
constexpr int TPB = 256;

// XCD-aware cell-block mapping for the gather-heavy sweeps: dispatch puts workgroup b on XCD
// b % 8, so hand XCD j the j-th contiguous eighth of the cell blocks -- neighbouring half-bricks
// then share one L2 instead of pulling the same fluid records into eight of them.  Grids are
// rounded up to a multiple of 8; returns -1 for the padding workgroups.
__device__ __forceinline__ int xcd_cell(int n_owned) {
  const int nblk = (n_owned + (int)blockDim.x - 1) / (int)blockDim.x;
  const int per = (nblk + 7) >> 3;
  const int b = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
  if (((int)blockIdx.x >> 3) >= per || b >= nblk) return -1;
  const int c = b * (int)blockDim.x + (int)threadIdx.x;
  return c < n_owned ? c : -1;
}

__device__ __forceinline__ double fd_step(double yv, double eps, double umin) {
  // MatFDColoring "ds" increment (doc/user/setup_time.rst:434-471)
  double dx = yv;
  if (fabs(dx) < umin) dx = (dx >= 0.0) ? umin : -umin;
  return dx * eps;
}

__device__ __forceinline__ void flag_error(int* flags, int cell) {
  atomicMax(&flags[0], 1);
  atomicMin(&flags[1], cell);
}

// ---- shared pieces of the cell-centric sweeps ------------------------------------------------
struct MeshView {
  const double* rock; const double* vol; const double* fgeom; const int* fdir;
  const int* adj_face; const int* adj_other; const int* adj_blk; const int* diag_blk;
  const int* adj_tblk;     // slot of THIS cell's column in the neighbour's block row (-1: the neighbour is no owned row)
  const int* cell_src;
  const int* src_next; const int* src_comp; const int* src_pcomp; const double* src_rate; const double* src_enth;
  SrcCtl* src_ctl;         // null: all rates as given (the unperturbed residual sweep notes threshold indices into the records)
  const double* src_net;   // null: no source network (source_network_rate)
  int n_owned, n_local, n_faces, max_deg;
};
static_assert(std::is_trivially_copyable<MeshView>::value, "a kernel argument holds views, never an owner");

__device__ __forceinline__ void load_face(const MeshView& m, int f, FaceGeom& g) {
  const size_t nf = m.n_faces;
  g.area = m.fgeom[f]; g.d1 = m.fgeom[nf + f]; g.d2 = m.fgeom[2 * nf + f];
  g.d12 = m.fgeom[3 * nf + f]; g.gn = m.fgeom[4 * nf + f]; g.dir = m.fdir[f];
}

// sign * (flux * area) / vol for the face in adjacency slot, evaluated with states (own, other)
template <int KIND>
__device__ __forceinline__ void slot_term(const FaceGeom& g, int side, const CellState<KIND>& own,
                                          const RockState& rown, const CellState<KIND>& oth,
                                          const RockState& roth, double vol, double* term) {
  using E = EosT<KIND>;
  double flux[E::np];
  if (side == 0) face_flux<KIND>(g, own, rown, oth, roth, flux);
  else face_flux<KIND>(g, oth, roth, own, rown, flux);
  const double sign = side ? 1.0 : -1.0;
#pragma unroll
  for (int k = 0; k < E::np; k++) term[k] = sign * (flux[k] * g.area) / vol;
}

template <int KIND>
__device__ __forceinline__ void source_terms(const MeshView& m, int c, const CellState<KIND>& s,
                                             double vol, double* R, bool commit = false) {
  using E = EosT<KIND>;
  for (int si = m.cell_src[c]; si >= 0; si = m.src_next[si]) {
    double flow[E::np];
    source_flow<KIND>(s, source_rate<KIND>(s, m.src_ctl, si, m.src_rate[si], m.src_net, commit), m.src_enth[si], m.src_comp[si], m.src_pcomp[si], flow);
#pragma unroll
    for (int k = 0; k < E::np; k++) R[k] += flow[k] / vol;
  }
}

// backwards_Euler_residual / BDF2_residual / direct_ss_residual (src/timestepper.F90:345-452) in
// the reference's order of operations; l1, l2 = lhs one and two steps back for this equation
__device__ __forceinline__ double res_form(const ResForm& rf, double L, double R, double l1, double l2) {
  if (rf.method == WAI_METHOD_BDF2) {
    const double r = rf.ratio, r1 = r + 1.0;
    double v = L * (1.0 + 2.0 * r);
    v = v + (-r1 * r1) * l1;
    v = v + (r * r) * l2;
    return v + (-rf.dt * r1) * R;
  }
  if (rf.method == WAI_METHOD_DIRECTSS) return R;
  return (L - l1) - rf.dt * R;
}

// ---- records parked in LDS (k_residual_tile, k_jacobian_park) ------------------------------------------
template <int KIND> struct ParkT {
  using E = EosT<KIND>;
  static constexpr int nld = 4 + E::nph * (7 + (E::nc > 1 ? E::nc : 0));   // doubles load_state reads
  // what a parked record holds: what the FLUX (and the source terms) read of a state -- not the internal energies, which
  // only the accumulation term uses, and the permeability factor only where it is not identically 1 (salt: halite)
  static constexpr int npark = 3 + (is_salt<KIND> ? 1 : 0) + E::nph * (6 + (E::nc > 1 ? E::nc : 0));
  static constexpr int threads = E::np <= 2 ? 128 : 64;
  // parked own-perturbed states + base terms of max_deg faces, per thread.  Round 4: the leaner record and max_deg instead
  // of a fixed 8 slots bring a 64-thread workgroup of 3 x 3 blocks from 46 080 to 39 936 B (eos wce, 6 or 7 faces): FOUR
  // workgroups per CU, one wave on every SIMD, where three left one SIMD idle
  static constexpr int lds_bytes(int max_deg) { return E::np * (npark + max_deg) * 8 * threads; }
  // three workgroups per CU or the plain kernel: MEASURED 13.7 -> 10.4 ms (we, 216^3), 12.5 -> 11.0 (wce,
  // 172x172x170; 14.7 with 128 threads = one workgroup per CU); the three-phase salt EOS would hold one
  static constexpr bool use = E::np * (npark + MAXDEG) * 8 * threads <= 54 * 1024;
};
template <int KIND>
__device__ __forceinline__ void park_state(const CellState<KIND>& s, double* __restrict__ b, int st) {
  using E = EosT<KIND>;
  int f = 0;
  b[(f++) * st] = s.P; b[(f++) * st] = s.T; b[(f++) * st] = s.phases;
  if constexpr (is_salt<KIND>) b[(f++) * st] = s.permfac;
#pragma unroll
  for (int p = 0; p < E::nph; p++) {
    b[(f++) * st] = s.rho[p]; b[(f++) * st] = s.mu[p]; b[(f++) * st] = s.sat[p]; b[(f++) * st] = s.kr[p];
    b[(f++) * st] = s.pc[p]; b[(f++) * st] = s.h[p];
    if constexpr (E::nc > 1) {
#pragma unroll
      for (int q = 0; q < E::nc; q++) b[(f++) * st] = s.x[p][q];
    }
  }
}
template <int KIND>
__device__ __forceinline__ void unpark_state(const double* __restrict__ b, int st, CellState<KIND>& s) {
  using E = EosT<KIND>;
  int f = 0;
  s.P = b[(f++) * st]; s.T = b[(f++) * st]; s.phases = b[(f++) * st];
  if constexpr (is_salt<KIND>) s.permfac = b[(f++) * st];
  else s.permfac = 1.0;   // eos_eval leaves it at 1 where no permeability modifier exists
  s.region = 0.0;
#pragma unroll
  for (int q = 0; q < E::nc; q++) s.pp[q] = 0.0;
#pragma unroll
  for (int p = 0; p < E::nph; p++) {
    s.rho[p] = b[(f++) * st]; s.mu[p] = b[(f++) * st]; s.sat[p] = b[(f++) * st]; s.kr[p] = b[(f++) * st];
    s.pc[p] = b[(f++) * st]; s.h[p] = b[(f++) * st]; s.u[p] = 0.0;   // (not read by the flux or the sources)
    if constexpr (E::nc == 1) {
      s.x[p][0] = (((int)s.phases >> p) & 1) ? 1.0 : 0.0;
    } else {
#pragma unroll
      for (int q = 0; q < E::nc; q++) s.x[p][q] = b[(f++) * st];
    }
  }
}

// ---- host side: what every launcher starts from -------------------------------------------------
static inline MeshView view(wai_ctx* c) {
  MeshView m;
  m.rock = c->mesh.rock; m.vol = c->mesh.vol; m.fgeom = c->mesh.fgeom; m.fdir = c->mesh.fdir;
  m.adj_face = c->mesh.adj_face; m.adj_other = c->mesh.adj_other; m.adj_blk = c->mesh.adj_blk;
  m.diag_blk = c->mesh.diag_blk; m.cell_src = c->mesh.cell_src; m.adj_tblk = c->mesh.adj_tblk;
  m.src_next = c->src.next; m.src_comp = c->src.comp; m.src_pcomp = c->src.pcomp; m.src_rate = c->src.rate;
  m.src_enth = c->src.enth; m.src_ctl = c->src.ctl; m.src_net = c->src.net;
  m.n_owned = c->mesh.n_owned; m.n_local = c->mesh.n_local; m.n_faces = c->mesh.n_faces;
  m.max_deg = c->mesh.max_deg;
  return m;
}

static inline int grid_for(size_t n) { return (int)((n + TPB - 1) / TPB); }
static inline int grid8_for(size_t n) { return ((grid_for(n) + 7) / 8) * 8; }  // xcd_cell kernels

static inline ResForm res_form_of(const wai_ctx* c, double dt, const double* lhs_old) {
  ResForm rf;
  rf.method = c->method;
  rf.dt = dt;
  rf.ratio = c->ratio;
  rf.last = lhs_old;
  rf.last2 = c->w_lhs2;
  return rf;
}

// After a launch: a refused one must not leave the kernel's outputs stale in silence -- its name and the runtime's
// reason go into c->err, and the launcher returns this -1.  No synchronisation: this sees the launch, not the run.
static inline int launched(wai_ctx* c, const char* kernel) {
  if (hipError_t e = hipGetLastError(); e != hipSuccess) { c->err = std::string(kernel) + ": " + hipGetErrorString(e); return -1; }
  return 0;
}

}  // namespace wai
