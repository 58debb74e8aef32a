// Assembly kernels: the finite-difference block-ELL Jacobian (K5).  k_jacobian_sym (column-wise off-diagonal blocks) is
// the default; the row-wise k_jacobian_park and k_jacobian remain behind WAI_JAC_SYM=0 / WAI_JAC_PARK=0, and the tests
// compare the three.  Shared pieces: assembly_device.hip.h.
#include "assembly_device.hip.h"

namespace wai {

// ---- K5: FD Jacobian, one block row per thread -----------------------------------------------
template <int KIND>
__global__ __launch_bounds__(TPB) void k_jacobian(MeshView m, const double* __restrict__ flu,
                                                  size_t stride, const double* __restrict__ flu_pert,
                                                  const double* __restrict__ hstep, int n_prim,
                                                  ResForm rf, double* __restrict__ val) {
  using E = EosT<KIND>;
  constexpr int np = E::np, bb = E::np * E::np;
  const int c = xcd_cell(m.n_owned);
  if (c < 0) return;
  CellState<KIND> own0;
  RockState rown;
  load_state<KIND>(flu, stride, c, own0);
  load_rock(m.rock, m.n_local, c, rown);
  const double vol = m.vol[c];
  double lold[np], lold2[np];
#pragma unroll
  for (int k = 0; k < np; k++) {
    lold[k] = rf.method == WAI_METHOD_DIRECTSS ? 0.0 : rf.last[(size_t)c * np + k];
    lold2[k] = rf.method == WAI_METHOD_BDF2 ? rf.last2[(size_t)c * np + k] : 0.0;
  }

  // base residual, keeping every slot's contribution
  double L0[np], terms0[MAXDEG][np], src0[np], f0[np];
  cell_balance<KIND>(own0, rown, L0);
#pragma unroll
  for (int s = 0; s < MAXDEG; s++) {
#pragma unroll
    for (int k = 0; k < np; k++) terms0[s][k] = 0.0;
    if (s < m.max_deg) {
      const int fs = m.adj_face[(size_t)s * m.n_owned + c];
      if (fs >= 0) {
        const int o = m.adj_other[(size_t)s * m.n_owned + c];
        FaceGeom g;
        load_face(m, fs >> 1, g);
        CellState<KIND> oth;
        RockState roth;
        load_state<KIND>(flu, stride, o, oth);
        load_rock(m.rock, m.n_local, o, roth);
        slot_term<KIND>(g, fs & 1, own0, rown, oth, roth, vol, terms0[s]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < np; k++) src0[k] = 0.0;
  source_terms<KIND>(m, c, own0, vol, src0);
  {
    double R[np];
#pragma unroll
    for (int k = 0; k < np; k++) R[k] = 0.0;
#pragma unroll
    for (int s = 0; s < MAXDEG; s++) {
      if (s < m.max_deg && m.adj_face[(size_t)s * m.n_owned + c] >= 0) {
#pragma unroll
        for (int k = 0; k < np; k++) R[k] += terms0[s][k];
      }
    }
#pragma unroll
    for (int k = 0; k < np; k++) { R[k] += src0[k]; f0[k] = res_form(rf, L0[k], R[k], lold[k], lold2[k]); }
  }

  // diagonal block: own state perturbed in component k
  // block-ELL planes: element (r, k) of the block in slot q of block-row c is val[ell_ix(np, n_owned, q, r, k, c)]
  // (context.hpp; linalg_device.hip.h, "Matrix entry addressing")
  const size_t nrow = m.n_owned;
  const int dq = m.diag_blk[c];
#pragma unroll
  for (int k = 0; k < np; k++) {
    CellState<KIND> ownk;
    load_state<KIND>(flu_pert + (size_t)k * E::df * n_prim, (size_t)n_prim, c, ownk);
    double Lk[np], R[np];
    cell_balance<KIND>(ownk, rown, Lk);
#pragma unroll
    for (int q = 0; q < np; q++) R[q] = 0.0;
    for (int s = 0; s < m.max_deg; s++) {
      const int fs = m.adj_face[(size_t)s * m.n_owned + c];
      if (fs < 0) continue;
      const int o = m.adj_other[(size_t)s * m.n_owned + c];
      FaceGeom g;
      load_face(m, fs >> 1, g);
      CellState<KIND> oth;
      RockState roth;
      load_state<KIND>(flu, stride, o, oth);
      load_rock(m.rock, m.n_local, o, roth);
      double term[np];
      slot_term<KIND>(g, fs & 1, ownk, rown, oth, roth, vol, term);
#pragma unroll
      for (int q = 0; q < np; q++) R[q] += term[q];
    }
    source_terms<KIND>(m, c, ownk, vol, R);
    const double h = hstep[(size_t)c * np + k];
#pragma unroll
    for (int r = 0; r < np; r++) {
      const double f1 = res_form(rf, Lk[r], R[r], lold[r], lold2[r]);
      __builtin_nontemporal_store((f1 - f0[r]) / h, val + ell_ix(np, nrow, dq, r, k, (size_t)c));
    }
  }

  // off-diagonal blocks: neighbour across slot s perturbed in component k
#pragma unroll
  for (int s = 0; s < MAXDEG; s++) {
    if (s >= m.max_deg) continue;
    const int fs = m.adj_face[(size_t)s * m.n_owned + c];
    if (fs < 0) continue;
    const int blk = m.adj_blk[(size_t)s * m.n_owned + c];
    if (blk < 0) continue;  // Dirichlet ghost: no column
    const int o = m.adj_other[(size_t)s * m.n_owned + c];
    FaceGeom g;
    load_face(m, fs >> 1, g);
    RockState roth;
    load_rock(m.rock, m.n_local, o, roth);
#pragma unroll
    for (int k = 0; k < np; k++) {
      CellState<KIND> othk;
      load_state<KIND>(flu_pert + (size_t)k * E::df * n_prim, (size_t)n_prim, o, othk);
      double term[np], R[np];
      slot_term<KIND>(g, fs & 1, own0, rown, othk, roth, vol, term);
#pragma unroll
      for (int q = 0; q < np; q++) R[q] = 0.0;
#pragma unroll
      for (int s2 = 0; s2 < MAXDEG; s2++) {
        if (s2 < m.max_deg && m.adj_face[(size_t)s2 * m.n_owned + c] >= 0) {
#pragma unroll
          for (int q = 0; q < np; q++) R[q] += (s2 == s) ? term[q] : terms0[s2][q];
        }
      }
      const double h = hstep[(size_t)o * np + k];
#pragma unroll
      for (int r = 0; r < np; r++) {
        const double f1 = res_form(rf, L0[r], R[r] + src0[r], lold[r], lold2[r]);
        __builtin_nontemporal_store((f1 - f0[r]) / h, val + ell_ix(np, nrow, blk, r, k, (size_t)c));
      }
    }
  }
}

// ---- K5': the same Jacobian with the own-perturbed states parked in LDS ---------------------------
// k_jacobian reads a neighbour's unperturbed state once for the base residual and once more for every
// own-perturbed evaluation (the perturbation loop is outside the face loop, because only one perturbed
// own state fits the registers next to the base state and the neighbour's).  None of these re-reads
// hits a cache: between two of them a wave streams ~140 KB and an XCD's 32 CUs ~36 MB through the 4 MB
// L2 (PMC: 9.6 KB of L2-miss traffic per cell = every load of the kernel).  Here the np own-perturbed
// states go to LDS once (np x 18-34 doubles per thread, field-major: conflict-free) and the face loop
// is outermost for the base and the own-perturbed evaluations together, so a neighbour's state, rock
// and face record are loaded once for all of them: 21 instead of 33 state records per cell for np = 2,
// 13 instead of 25 rock records, 12 instead of 24 face records.  Same evaluations, same summation
// order, bit-identical blocks.
template <int KIND>
__global__ __launch_bounds__(ParkT<KIND>::threads, (EosT<KIND>::np <= 2 ? 2 : 1)) void k_jacobian_park(MeshView m, const double* __restrict__ flu,
                                                  size_t stride, const double* __restrict__ flu_pert,
                                                  const double* __restrict__ hstep, int n_prim,
                                                  ResForm rf, double* __restrict__ val) {
  using E = EosT<KIND>;
  constexpr int np = E::np, bb = E::np * E::np;
  const int c = xcd_cell(m.n_owned);
  if (c < 0) return;
  CellState<KIND> own0;
  RockState rown;
  load_state<KIND>(flu, stride, c, own0);
  load_rock(m.rock, m.n_local, c, rown);
  const double vol = m.vol[c];
  double lold[np], lold2[np];
#pragma unroll
  for (int k = 0; k < np; k++) {
    lold[k] = rf.method == WAI_METHOD_DIRECTSS ? 0.0 : rf.last[(size_t)c * np + k];
    lold2[k] = rf.method == WAI_METHOD_BDF2 ? rf.last2[(size_t)c * np + k] : 0.0;
  }

  // own-perturbed states: accumulation terms now, the states themselves into LDS (thread-private columns)
  extern __shared__ double park[];
  constexpr int nld = ParkT<KIND>::npark;
  const int st = (int)blockDim.x;
  double Lk[np][np], Rk[np][np];
#pragma unroll
  for (int k = 0; k < np; k++) {
    CellState<KIND> ownk;
    load_state<KIND>(flu_pert + (size_t)k * E::df * n_prim, (size_t)n_prim, c, ownk);
    cell_balance<KIND>(ownk, rown, Lk[k]);
    park_state<KIND>(ownk, park + (size_t)k * nld * st + threadIdx.x, st);
#pragma unroll
    for (int q = 0; q < np; q++) Rk[k][q] = 0.0;
  }
  // base residual, keeping every slot's contribution (in LDS too: [slot][component][thread], so that the
  // face loops need not be unrolled); the own-perturbed evaluations of the same face with it
  double* terms0 = park + (size_t)np * nld * st + threadIdx.x;
  double L0[np], src0[np], f0[np];
  cell_balance<KIND>(own0, rown, L0);
  unsigned valid = 0u;
#pragma unroll 1
  for (int s = 0; s < m.max_deg; s++) {
    const int fs = m.adj_face[(size_t)s * m.n_owned + c];
    if (fs < 0) continue;
    valid |= 1u << s;
    const int o = m.adj_other[(size_t)s * m.n_owned + c];
    FaceGeom g;
    load_face(m, fs >> 1, g);
    CellState<KIND> oth;
    RockState roth;
    load_state<KIND>(flu, stride, o, oth);
    load_rock(m.rock, m.n_local, o, roth);
    double t0[np];
    slot_term<KIND>(g, fs & 1, own0, rown, oth, roth, vol, t0);
#pragma unroll
    for (int q = 0; q < np; q++) terms0[(size_t)(s * np + q) * st] = t0[q];
#pragma unroll
    for (int k = 0; k < np; k++) {
      CellState<KIND> ownk;
      unpark_state<KIND>(park + (size_t)k * nld * st + threadIdx.x, st, ownk);
      double term[np];
      slot_term<KIND>(g, fs & 1, ownk, rown, oth, roth, vol, term);
#pragma unroll
      for (int q = 0; q < np; q++) Rk[k][q] += term[q];
    }
  }
#pragma unroll
  for (int k = 0; k < np; k++) src0[k] = 0.0;
  source_terms<KIND>(m, c, own0, vol, src0);
  {
    double R[np];
#pragma unroll
    for (int k = 0; k < np; k++) R[k] = 0.0;
#pragma unroll 1
    for (int s = 0; s < m.max_deg; s++) {
      if ((valid >> s) & 1u) {
#pragma unroll
        for (int k = 0; k < np; k++) R[k] += terms0[(size_t)(s * np + k) * st];
      }
    }
#pragma unroll
    for (int k = 0; k < np; k++) { R[k] += src0[k]; f0[k] = res_form(rf, L0[k], R[k], lold[k], lold2[k]); }
  }

  // diagonal block: own state perturbed in component k
  // block-ELL planes: element (r, k) of the block in slot q of block-row c is val[ell_ix(np, n_owned, q, r, k, c)]
  // (context.hpp; linalg_device.hip.h, "Matrix entry addressing")
  const size_t nrow = m.n_owned;
  const int dq = m.diag_blk[c];
#pragma unroll
  for (int k = 0; k < np; k++) {
    CellState<KIND> ownk;
    unpark_state<KIND>(park + (size_t)k * nld * st + threadIdx.x, st, ownk);
    source_terms<KIND>(m, c, ownk, vol, Rk[k]);
    const double h = hstep[(size_t)c * np + k];
#pragma unroll
    for (int r = 0; r < np; r++) {
      const double f1 = res_form(rf, Lk[k][r], Rk[k][r], lold[r], lold2[r]);
      __builtin_nontemporal_store((f1 - f0[r]) / h, val + ell_ix(np, nrow, dq, r, k, (size_t)c));
    }
  }

  // off-diagonal blocks: neighbour across slot s perturbed in component k.  SHARE (128-thread workgroups, np <= 2): a
  // neighbour that belongs to this workgroup has its perturbed states in LDS already -- they are what its thread parked
  // -- so they are taken from there instead of memory (MEASURED, round 3: 10.38 -> 10.05 ms at 216^3; the 64-thread
  // workgroups of 3 x 3 blocks hold few of their own neighbours and lose to the divergent branch: 11.1 -> 12.3 ms at C4)
  constexpr bool SHARE = np <= 2;
  const int c0 = c - (int)threadIdx.x, c1 = min(c0 + st, m.n_owned);
  if constexpr (SHARE) __syncthreads();   // every thread's states are parked
#pragma unroll 1
  for (int s = 0; s < m.max_deg; s++) {
    if (!((valid >> s) & 1u)) continue;
    const int blk = m.adj_blk[(size_t)s * m.n_owned + c];
    if (blk < 0) continue;  // Dirichlet ghost: no column
    const int fs = m.adj_face[(size_t)s * m.n_owned + c];
    const int o = m.adj_other[(size_t)s * m.n_owned + c];
    FaceGeom g;
    load_face(m, fs >> 1, g);
    RockState roth;
    load_rock(m.rock, m.n_local, o, roth);
#pragma unroll
    for (int k = 0; k < np; k++) {
      CellState<KIND> othk;
      if (SHARE && o >= c0 && o < c1) unpark_state<KIND>(park + (size_t)k * nld * st + (o - c0), st, othk);   // what its thread parked
      else load_state<KIND>(flu_pert + (size_t)k * E::df * n_prim, (size_t)n_prim, o, othk);
      double term[np], R[np];
      slot_term<KIND>(g, fs & 1, own0, rown, othk, roth, vol, term);
#pragma unroll
      for (int q = 0; q < np; q++) R[q] = 0.0;
#pragma unroll 1
      for (int s2 = 0; s2 < m.max_deg; s2++) {
        if ((valid >> s2) & 1u) {
#pragma unroll
          for (int q = 0; q < np; q++) R[q] += (s2 == s) ? term[q] : terms0[(size_t)(s2 * np + q) * st];
        }
      }
      const double h = hstep[(size_t)o * np + k];
#pragma unroll
      for (int r = 0; r < np; r++) {
        const double f1 = res_form(rf, L0[r], R[r] + src0[r], lold[r], lold2[r]);
        __builtin_nontemporal_store((f1 - f0[r]) / h, val + ell_ix(np, nrow, blk, r, k, (size_t)c));
      }
    }
  }
}

// ---- K5, column-wise off-diagonal blocks (round 5) ---------------------------------------------------------------
// k_jacobian / k_jacobian_park difference every ROW: for its off-diagonal block (c, o) the thread of cell c fetches the
// np perturbed states of neighbour o, so every cell's base + np perturbed records are read by the cell itself and by
// its six neighbours -- 21 records of 144 B per cell for eos we, none of the re-reads hits (the working set of an XCD's
// resident workgroups is larger than its 4-MB L2): 40 GB per launch at 216^3, 7.8 x the algorithmic bytes.
// The face flux F(c1, c2) is ONE function of the two states for both rows it feeds (+ F A / V in one, - F A / V in the
// other), and the evaluation with c's k-th perturbed state that row c needs for its diagonal block is the very
// evaluation row o needs for its block (o, c).  So here the thread of cell c evaluates every face with its own base
// and perturbed states against the neighbour's BASE state only -- 3 + 6 = 9 records per cell -- and produces its
// diagonal block AND column c of every neighbouring row: block (o, c) = dR (term_o(pert_c^k) - term_o(base)) / h_ck,
// term_o = -+ (F A) / V_o the neighbour's slot term (the same expression k_residual evaluates for row o, from the same
// flux), dR = d res_form / d R (-dt for backward Euler).  Each off-diagonal block is still produced by exactly one
// thread and STORED; blocks whose column cell has no thread on this rank (partition ghosts) are produced by the row's
// thread from the ghost's perturbed records, by the same formula.
// The diagonal block is the literal difference of the whole row's residual, bit for bit as before.  An off-diagonal
// entry differs from the literal (f_o(y + h e) - f_o(y)) / h by the rounding of that difference of sums,
// <= a few eps |f_o| / h -- inside the parity bar (tests/test_hip_parity.py::test_jacobian: 2e-5 of the block row's
// scale; bench.py's check: max of that and 16 eps |L| / h), and by construction the MORE accurate of the two.
template <int KIND>
__device__ __forceinline__ void slot_flux(const FaceGeom& g, int side, const CellState<KIND>& own,
                                          const RockState& rown, const CellState<KIND>& oth,
                                          const RockState& roth, double* flux) {
  if (side == 0) face_flux<KIND>(g, own, rown, oth, roth, flux);
  else face_flux<KIND>(g, oth, roth, own, rown, flux);
}
__device__ __forceinline__ double res_dR(const ResForm& rf) {   // d res_form / d R
  if (rf.method == WAI_METHOD_BDF2) return -rf.dt * (rf.ratio + 1.0);
  if (rf.method == WAI_METHOD_DIRECTSS) return 1.0;
  return -rf.dt;
}
// waves per SIMD the np <= 2 kernel is built for: MEASURED at 216^3 (profiles/jsym_waves_ab_r5.log) 1 (no scratch, 282 registers)
// 6.0 ms, 2 (256 VGPRs + 104 B of scratch per lane) 5.14 ms, 3 (168 VGPRs, 428 B) 9.75 ms
constexpr int JSYM_WAVES = 2;
template <int KIND>
__global__ __launch_bounds__(ParkT<KIND>::threads, (EosT<KIND>::np <= 2 ? JSYM_WAVES : 1)) void k_jacobian_sym(MeshView m, const double* __restrict__ flu,
                                                  size_t stride, const double* __restrict__ flu_pert,
                                                  const double* __restrict__ hstep, int n_prim,
                                                  ResForm rf, double* __restrict__ val) {
  using E = EosT<KIND>;
  constexpr int np = E::np;
  const int c = xcd_cell(m.n_owned);
  if (c < 0) return;
  CellState<KIND> own0;
  RockState rown;
  load_state<KIND>(flu, stride, c, own0);
  load_rock(m.rock, m.n_local, c, rown);
  const double vol = m.vol[c];
  double hk[np];
#pragma unroll
  for (int k = 0; k < np; k++) hk[k] = hstep[(size_t)c * np + k];
  extern __shared__ double park[];
  constexpr int nld = ParkT<KIND>::npark;
  const int st = (int)blockDim.x;
  double Rk[np][np];
  double* lpark = park + (size_t)np * nld * st + threadIdx.x;     // the perturbed states' accumulation terms wait in LDS too
#pragma unroll
  for (int k = 0; k < np; k++) {
    CellState<KIND> ownk;
    double Lk[np];
    load_state<KIND>(flu_pert + (size_t)k * E::df * n_prim, (size_t)n_prim, c, ownk);
    cell_balance<KIND>(ownk, rown, Lk);
    park_state<KIND>(ownk, park + (size_t)k * nld * st + threadIdx.x, st);
#pragma unroll
    for (int q = 0; q < np; q++) { lpark[(size_t)(k * np + q) * st] = Lk[q]; Rk[k][q] = 0.0; }
  }
  const size_t nrow = m.n_owned;
  const double dR = res_dR(rf);
  double L0[np], R0[np], f0[np];
  cell_balance<KIND>(own0, rown, L0);
  bool ghost_cols = false;
#pragma unroll
  for (int k = 0; k < np; k++) R0[k] = 0.0;
#pragma unroll 1
  for (int s = 0; s < m.max_deg; s++) {
    const int fs = m.adj_face[(size_t)s * m.n_owned + c];
    if (fs < 0) continue;
    const int o = m.adj_other[(size_t)s * m.n_owned + c];
    const int tb = m.adj_tblk[(size_t)s * m.n_owned + c];   // >= 0: o is an owned row and this is the slot of column c in it
    FaceGeom g;
    load_face(m, fs >> 1, g);
    CellState<KIND> oth;
    RockState roth;
    load_state<KIND>(flu, stride, o, oth);
    load_rock_face(m.rock, m.n_local, o, g.dir, roth);
    const int side = fs & 1;
    const double sign = side ? 1.0 : -1.0;
    const double volo = tb >= 0 ? m.vol[o] : 1.0;
    double fl0[np], to0[np];
    slot_flux<KIND>(g, side, own0, rown, oth, roth, fl0);
#pragma unroll
    for (int q = 0; q < np; q++) {
      R0[q] += sign * (fl0[q] * g.area) / vol;            // slot_term's expression, this row's side ...
      to0[q] = -sign * (fl0[q] * g.area) / volo;          // ... and the neighbour's
    }
#pragma unroll
    for (int k = 0; k < np; k++) {
      CellState<KIND> ownk;
      unpark_state<KIND>(park + (size_t)k * nld * st + threadIdx.x, st, ownk);
      double fl[np];
      slot_flux<KIND>(g, side, ownk, rown, oth, roth, fl);
#pragma unroll
      for (int q = 0; q < np; q++) Rk[k][q] += sign * (fl[q] * g.area) / vol;
      if (tb >= 0) {
#pragma unroll
        for (int r = 0; r < np; r++) {
          const double tok = -sign * (fl[r] * g.area) / volo;
          val[ell_ix(np, nrow, tb, r, k, (size_t)o)] = dR * (tok - to0[r]) / hk[k];
        }
      }
    }
    ghost_cols |= (m.adj_blk[(size_t)s * m.n_owned + c] >= 0 && o >= m.n_owned);
  }
  // column cells without a thread on this rank (partition ghosts; none on one rank): block (c, o) from the ghost's
  // perturbed records, in a loop of its own so that the sweep above does not carry its registers
  if (ghost_cols) {
#pragma unroll 1
    for (int s = 0; s < m.max_deg; s++) {
      const int fs = m.adj_face[(size_t)s * m.n_owned + c];
      if (fs < 0) continue;
      const int o = m.adj_other[(size_t)s * m.n_owned + c];
      const int blk = m.adj_blk[(size_t)s * m.n_owned + c];
      if (blk < 0 || o < m.n_owned) continue;
      FaceGeom g;
      load_face(m, fs >> 1, g);
      CellState<KIND> oth;
      RockState roth;
      load_state<KIND>(flu, stride, o, oth);
      load_rock_face(m.rock, m.n_local, o, g.dir, roth);
      const int side = fs & 1;
      const double sign = side ? 1.0 : -1.0;
      double fl0[np];
      slot_flux<KIND>(g, side, own0, rown, oth, roth, fl0);
#pragma unroll 1
      for (int k = 0; k < np; k++) {
        load_state<KIND>(flu_pert + (size_t)k * E::df * n_prim, (size_t)n_prim, o, oth);
        double fl[np];
        slot_flux<KIND>(g, side, own0, rown, oth, roth, fl);
        const double h = hstep[(size_t)o * np + k];
#pragma unroll
        for (int r = 0; r < np; r++) {
          const double t1 = sign * (fl[r] * g.area) / vol, t0 = sign * (fl0[r] * g.area) / vol;
          __builtin_nontemporal_store(dR * (t1 - t0) / h, val + ell_ix(np, nrow, blk, r, k, (size_t)c));
        }
      }
    }
  }
  double src0[np];
#pragma unroll
  for (int k = 0; k < np; k++) src0[k] = 0.0;
  source_terms<KIND>(m, c, own0, vol, src0);
  // (the earlier steps' accumulation terms only enter here: loaded behind the face loop, which is short of registers)
  double lold[np], lold2[np];
#pragma unroll
  for (int k = 0; k < np; k++) {
    lold[k] = rf.method == WAI_METHOD_DIRECTSS ? 0.0 : rf.last[(size_t)c * np + k];
    lold2[k] = rf.method == WAI_METHOD_BDF2 ? rf.last2[(size_t)c * np + k] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < np; k++) { R0[k] += src0[k]; f0[k] = res_form(rf, L0[k], R0[k], lold[k], lold2[k]); }
  // diagonal block: the literal difference of the row's residual, as k_jacobian_park forms it
  const int dq = m.diag_blk[c];
#pragma unroll
  for (int k = 0; k < np; k++) {
    CellState<KIND> ownk;
    unpark_state<KIND>(park + (size_t)k * nld * st + threadIdx.x, st, ownk);
    source_terms<KIND>(m, c, ownk, vol, Rk[k]);
#pragma unroll
    for (int r = 0; r < np; r++) {
      const double f1 = res_form(rf, lpark[(size_t)(k * np + r) * st], Rk[k][r], lold[r], lold2[r]);
      __builtin_nontemporal_store((f1 - f0[r]) / hk[k], val + ell_ix(np, nrow, dq, r, k, (size_t)c));
    }
  }
}

// ---- launcher --------------------------------------------------------------------------------
int launch_jacobian(wai_ctx* c, double dt, const double* lhs_old) {
  const MeshView m = view(c);
  const size_t stride = c->mesh.n_local;
  const ResForm rf = res_form_of(c, dt, lhs_old);
  // No clearing pass and no read-modify-write: two cells share at most one face (wai_ctx_create refuses duplicate
  // connections), so every block of a row is produced by exactly one adjacency slot and is STORED; the padding slots of
  // the block-ELL planes were zeroed once at creation and nobody writes them.  (Rounds 1-3 zeroed the 2.5 GB of a
  // 216^3 matrix before every assembly and accumulated into it: 4.6 GB of the launch's traffic.)
  const char* ep = getenv("WAI_JAC_PARK");   // read per call: tests compare the two kernels in one process
  const bool park = !(ep && ep[0] == '0');
  // column-wise off-diagonal blocks (k_jacobian_sym): 3 + 6 instead of 3 + 6 (1 + np) state records per cell and 1 + np
  // instead of 1 + 2 np flux evaluations per face.  MEASURED (profiles/asm_traffic_r5_*.log, same box): 9.59 -> 5.26 ms and
  // 40.0 -> 26.3 GB at C3 (eos we), 7.34 -> 3.81 ms / 24.3 -> 11.7 GB at C4 (wce), 3.06 -> 1.54 ms / 5.7 -> 3.7 GB at C5.
  // The default for every EOS; WAI_JAC_SYM=0 takes the row-wise kernels (read per call: tests compare them in one process)
  const char* es = getenv("WAI_JAC_SYM");
  const bool sym = park && c->mesh.adj_tblk && (es ? es[0] == '1' : true);
  const char* kernel = nullptr;   // what was launched (null: refused before any launch, c->err says why)
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        constexpr int T = ParkT<K>::threads;
        constexpr int sym_lds = EosT<K>::np * (ParkT<K>::npark + EosT<K>::np) * 8 * T;
        const int g = (((int)((m.n_owned + T - 1) / T) + 7) / 8) * 8;   // T-thread workgroups, xcd_cell's multiple of 8
        // the parked records of k_jacobian_sym must fit the LDS a workgroup may ask for (72 KB for the four-equation salt
        // EOS: fine on gfx950)
        if (sym && (size_t)sym_lds <= c->lds_per_block) {
          kernel = "k_jacobian_sym";
          hipLaunchKernelGGL(k_jacobian_sym<K>, g, T, sym_lds, c->stream, m, c->flu, stride, c->flu_pert, c->hstep,
                             c->mesh.n_prim, rf, c->flow.A.val);
          return;
        }
        // the row-wise kernels hold the base terms of MAXDEG faces per cell in registers / LDS: cells with more faces (up
        // to 16, wai_ctx_create) are assembled column-wise only
        if (m.max_deg > MAXDEG) {
          c->err = "the row-wise Jacobian (WAI_JAC_SYM=0) supports cells with at most 8 faces; this mesh has a cell with " +
                   std::to_string(m.max_deg) + " (the default column-wise Jacobian takes up to 16)";
          return;
        }
        if (park && ParkT<K>::use) {   // (a run-time test: k_jacobian_park<K> exists for every EOS)
          kernel = "k_jacobian_park";
          hipLaunchKernelGGL(k_jacobian_park<K>, g, T, ParkT<K>::lds_bytes(m.max_deg), c->stream, m, c->flu, stride,
                             c->flu_pert, c->hstep, c->mesh.n_prim, rf, c->flow.A.val);
        } else {
          kernel = "k_jacobian";
          hipLaunchKernelGGL(k_jacobian<K>, grid8_for(m.n_owned), TPB, 0, c->stream, m, c->flu, stride, c->flu_pert, c->hstep,
                             c->mesh.n_prim, rf, c->flow.A.val);
        }
      })) return -1;
  return kernel ? launched(c, kernel) : -1;
}

}  // namespace wai
