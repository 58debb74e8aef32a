// Block-sparse linear algebra for gfx950: block SpMV (K6), block-Jacobi ILU(0) factor / apply
// (K7/K8), fused Krylov vector kernels and reductions (K9), halo pack/unpack.
//
// These replace what the reference gets from PETSc 3.22.5 (not vendored): MatMult_SeqBAIJ_N /
// MPIBAIJ, PCBJACOBI+PCILU(0) MatSolve_SeqBAIJ_N, and the VecDot/VecAXPY family inside KSPBCGS
// / KSPGMRES -- configured at src/timestepper.F90:1645-1836.  fp64, HBM-bound, no MFMA.
//
// Layout: block-ELL, slot-major struct-of-arrays (context.hpp).  Every kernel here is
// one-thread-per-block-row; thread i of a wave reads element i of a slot/entry plane, so each
// wave instruction moves 64 consecutive doubles (512 B) -- the matrix streams through at HBM
// rate with no LDS staging, and x is gathered through L2 (brick-major numbering keeps a row's
// neighbours within a few KB).  Workgroup -> row-range mapping is XCD-aware: block b runs on
// XCD b % 8, so XCD j is handed the j-th contiguous eighth of the rows / subdomains and its L2
// only ever holds that eighth's x entries.
//
// Preconditioner: one workgroup per block-Jacobi subdomain (a brick of the mesh, <= 1024
// rows), one thread per row.  The fused kernel k_pc computes t = A x for the subdomain's rows
// (optional), parks t in LDS, pulls the thread's factor row into registers, then runs the
// forward and backward substitutions level by level out of LDS with workgroup barriers only
// (levels = dependency depth inside the brick, computed once on the host).  The dot products
// BiCGStab needs of the result are reduced in the same kernel.
//
// This header: what every linear-algebra kernel shares -- the wave sum, the XCD mapping, the matrix-entry addressing and
// loads, the row product and the small dense helpers.  The kernels live in kernels_matrix.hip, kernels_factor.hip and
// kernels_fused.hip.
#pragma once
#include "context.hpp"

namespace wai {

constexpr int TPB = 256;

// The sum of a wave's 64 doubles, in every lane, by DPP row operations (row_shr 1, 2, 4, 8 inside the rows of 16, then
// row_bcast 15 and 31 across them) on the two halves of the double: six adds whose operands come through the VALU's
// data-parallel-primitive path instead of six dependent ds_bpermute round trips through the LDS pipe -- which the
// substitution sweeps of the other bricks on the CU are waiting on.  (Round 3 measured 0.6 % for the one or two sums of
// its launches and left the shuffle tree; the merged BiCGStab reductions make five per brick.)  Lanes without a source
// take 0.0, the identity; the order of the additions is fixed, so the sum is reproducible.
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double dpp_add(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, BANK_MASK, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, BANK_MASK, false);
  return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v) {
#ifdef WAI_SHFL_SUMS   // the shuffle tree of rounds 1-3 (A/B builds)
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return __shfl(v, 0);
#else
  v = dpp_add<0x111, 0xf, 0xf>(v);   // row_shr:1
  v = dpp_add<0x112, 0xf, 0xf>(v);   // row_shr:2
  v = dpp_add<0x114, 0xf, 0xe>(v);   // row_shr:4, lanes 4 .. 15 of a row
  v = dpp_add<0x118, 0xf, 0xc>(v);   // row_shr:8, lanes 8 .. 15: lane 15 holds its row's sum
  v = dpp_add<0x142, 0xa, 0xf>(v);   // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xc, 0xf>(v);   // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's sum
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
#endif
}
constexpr int WMAX = 8;  // block-ELL width handled in registers (7-point stencil: 7, MINC: 8)
constexpr int WMAX_WIDE = MAX_CELL_FACES;  // widest row of the wide kernels (k_spmv_wide, k_pc_wide): cells with up to 16 faces


__device__ __forceinline__ int xcd_remap(int b, int n) {
  // dispatch places block b on XCD b % 8: give XCD j the contiguous range j*per .. (j+1)*per
  const int per = (n + 7) >> 3;
  return (b & 7) * per + (b >> 3);
}

// Matrix entry addressing (ell_ix, context.hpp).  Block sizes 1 and 2: planes are indexed by (slot,
// row-in-block) and element i of a plane is the BS-vector holding that block row of block-row i,
// val[((s*BS + r)*n + i)*BS + k] -- for BS = 2 a lane's access is one 16-byte double2 and a wave
// instruction moves 1 KiB.  Block sizes >= 3: element by element -- a 24-byte block row per lane costs a dwordx4 and a
// dwordx2 that each touch every 128-byte line, MEASURED 5.5 TB/s streaming against 6.2-6.4 TB/s where every wave
// instruction reads 512 contiguous bytes of ONE block element (tools/micro/layout_bs3.hip).  Rounds 2-3 kept one plane
// per element, val[((s*BS + r)*BS + k)*n + i]; since the end of round 4 the BS^2 elements of 64 consecutive rows sit
// together inside the slot, val[s BS^2 ld + ((i/64) BS^2 + r BS + k) 64 + i%64] with ld = ell_ld(n): the same 512-byte
// accesses, but a slot is one stream of 4.6-KB runs instead of nine planes 40 MB apart (context.hpp).
template <int BS>
__device__ __forceinline__ size_t vix(int n, int s, int e, int i) {
  return ell_ix(BS, (size_t)n, s, e / BS, e % BS, (size_t)i);
}
// element e of block row i in an array of ONE block per row (the inverted pivots)
template <int BS>
__device__ __forceinline__ size_t dix(int n, int e, int i) {
  return ell_ix1(BS, (size_t)n, e / BS, e % BS, (size_t)i);
}
// load the BS x BS block (slot s, block row i) into b[].  The matrix (values, column indices) is
// read once per launch and the result vector written once: these streams carry the non-temporal
// hint so that they do not evict the vector segments the neighbour gathers want to find in L2
// (MEASURED at 216^3, same box: k_spmv 0.557 -> 0.441 ms = 82 % of 8 TB/s, k_pc_park 0.684 ->
// 0.654 ms, and with the BiCGStab vector updates hinted too 7.5 % per Newton step).
typedef double wai_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int load_col(const int* __restrict__ col, size_t idx) {
  return __builtin_nontemporal_load(col + idx);
}
__device__ __forceinline__ void store_z2(double* __restrict__ z, size_t i, double a, double b) {
  wai_d2 v = {a, b};
  __builtin_nontemporal_store(v, reinterpret_cast<wai_d2*>(z + i * 2));
}
template <int BS>
__device__ __forceinline__ void load_block(const double* __restrict__ val, int n, int s, int i, double* b) {
  if constexpr (BS == 2) {
    const size_t i0 = ell_ix(2, (size_t)n, s, 0, 0, (size_t)i), i1 = ell_ix(2, (size_t)n, s, 1, 0, (size_t)i);
    const wai_d2 r0 = __builtin_nontemporal_load(reinterpret_cast<const wai_d2*>(val + i0));
    const wai_d2 r1 = __builtin_nontemporal_load(reinterpret_cast<const wai_d2*>(val + i1));
    b[0] = r0.x; b[1] = r0.y; b[2] = r1.x; b[3] = r1.y;
  } else {
#pragma unroll
    for (int e = 0; e < BS * BS; e++) b[e] = val[vix<BS>(n, s, e, i)];
  }
}

// the block of row i in an array of one block per row (the inverted pivots: ell_ix1)
template <int BS>
__device__ __forceinline__ void load_pivot(const double* __restrict__ val, int n, int i, double* b) {
  if constexpr (BS <= 2) load_block<BS>(val, n, 0, i, b);
  else {
#pragma unroll
    for (int e = 0; e < BS * BS; e++) b[e] = val[dix<BS>(n, e, i)];
  }
}

// a 16-byte pair of doubles at 8-byte alignment: gfx950 serves it with one global_load_dwordx4 (unaligned access
// mode), so the three components of a 3 x 3 system's vector entry cost a dwordx4 + a dwordx2 instead of three
// dwordx2 gathers through the same cache lines (the three scalar gathers of rounds 1-2)
typedef double wai_d2u __attribute__((ext_vector_type(2), aligned(8)));
template <int BS>
__device__ __forceinline__ void load_x(const double* __restrict__ x, int col, double* xv) {
  if constexpr (BS == 2) {
    const double2 t = *reinterpret_cast<const double2*>(x + (size_t)col * 2);
    xv[0] = t.x; xv[1] = t.y;
  } else if constexpr (BS == 3) {
    const double* p = x + (size_t)col * 3;
    const wai_d2u t = *reinterpret_cast<const wai_d2u*>(p);
    xv[0] = t.x; xv[1] = t.y; xv[2] = p[2];
  } else if constexpr (BS == 4) {
    const double* p = x + (size_t)col * 4;
    const wai_d2u t = *reinterpret_cast<const wai_d2u*>(p), u = *reinterpret_cast<const wai_d2u*>(p + 2);
    xv[0] = t.x; xv[1] = t.y; xv[2] = u.x; xv[3] = u.y;
  } else {
#pragma unroll
    for (int k = 0; k < BS; k++) xv[k] = x[(size_t)col * BS + k];
  }
}

// The fused kernels' input composed on the fly (AX): x = in + nalpha * in2, one fused multiply-add per entry -- BiCGStab's
// S = R - alpha V is then never written to memory: the second fused launch of an iteration gathers R and V (own row and
// neighbours; the neighbours' lines are L2 hits either way) instead of reading an S that a separate launch had to write
// (k_bcgs_s: R, V read, S written).  The same fma as k_bcgs_s and k_bcgs_xrp use: identical bits wherever S is formed.
template <int BS, bool AX>
__device__ __forceinline__ void load_xs(const double* __restrict__ in, const double* __restrict__ in2, double nalpha,
                                        int col, double* xv) {
  load_x<BS>(in, col, xv);
  if constexpr (AX) {
    double x2[BS];
    load_x<BS>(in2, col, x2);
#pragma unroll
    for (int k = 0; k < BS; k++) xv[k] = __builtin_fma(nalpha, x2[k], xv[k]);
  }
}

template <int BS>
__device__ __forceinline__ void load_x_stream(const double* __restrict__ x, int col, double* xv) {   // read once
  if constexpr (BS == 2) {
    const wai_d2 t = __builtin_nontemporal_load(reinterpret_cast<const wai_d2*>(x + (size_t)col * 2));
    xv[0] = t.x; xv[1] = t.y;
  } else {
#pragma unroll
    for (int k = 0; k < BS; k++) xv[k] = x[(size_t)col * BS + k];
  }
}

// acc += A_row(i) * x over the W slots of block row i.
// Every slot sits behind its own `s < W` branch, and the compiler ends each with s_waitcnt vmcnt(0): a row's slots are
// streamed one after the other.  MEASURED (round 4, profiles/spmv_w7_ab_r4.log): a branch-free loop for W = 7, where all
// of a row's blocks and gathers are requested before the first is used, is SLOWER -- 0.480-0.484 against 0.438-0.464 ms
// at 216^3 (2 x 2 blocks), 0.565-0.575 against 0.496-0.510 at C4 (3 x 3) -- one slot's element planes at a time are 4 or
// 9 concurrent streams through the memory channels, all seven slots' 28 or 63.
// WM: the most slots a row may have (WMAX; WMAX_WIDE for the meshes whose cells have up to 16 faces)
template <int BS, int WM = WMAX>
__device__ __forceinline__ void ell_row_mult(int n, int W, int i, const int* __restrict__ col,
                                             const double* __restrict__ val,
                                             const double* __restrict__ x, double* acc) {
  constexpr int BB = BS * BS;
  int cs[WM];   // all column indices first: one round trip instead of one per slot
#pragma unroll
  for (int s = 0; s < WM; s++) {
    cs[s] = i;
    if (s < W) cs[s] = load_col(col, (size_t)s * n + i);
  }
#pragma unroll
  for (int s = 0; s < WM; s++) {
    if (s < W) {
      const int c = cs[s];
      double xv[BS], a[BS * BS];
      load_x<BS>(x, c, xv);
      load_block<BS>(val, n, s, i, a);
#pragma unroll
      for (int r = 0; r < BS; r++)
#pragma unroll
        for (int k = 0; k < BS; k++) acc[r] += a[r * BS + k] * xv[k];
    }
  }
}

// ---- small dense helpers ---------------------------------------------------------------------
template <int BS>
__device__ __forceinline__ bool block_inverse(const double* a, double* inv) {
  // Gauss-Jordan with partial pivoting, fully unrolled in registers
  double m[BS][2 * BS];
#pragma unroll
  for (int r = 0; r < BS; r++)
#pragma unroll
    for (int c = 0; c < BS; c++) { m[r][c] = a[r * BS + c]; m[r][BS + c] = (r == c) ? 1.0 : 0.0; }
  bool ok = true;
#pragma unroll
  for (int p = 0; p < BS; p++) {
    int piv = p;
#pragma unroll
    for (int r = p + 1; r < BS; r++)
      if (fabs(m[r][p]) > fabs(m[piv][p])) piv = r;
#pragma unroll
    for (int r = p + 1; r < BS; r++)
      if (r == piv) {
#pragma unroll
        for (int c = 0; c < 2 * BS; c++) { const double t = m[p][c]; m[p][c] = m[r][c]; m[r][c] = t; }
      }
    if (m[p][p] == 0.0) ok = false;
    const double d = 1.0 / m[p][p];
#pragma unroll
    for (int c = 0; c < 2 * BS; c++) m[p][c] *= d;
#pragma unroll
    for (int r = 0; r < BS; r++)
      if (r != p) {
        const double f = m[r][p];
#pragma unroll
        for (int c = 0; c < 2 * BS; c++) m[r][c] -= f * m[p][c];
      }
  }
#pragma unroll
  for (int r = 0; r < BS; r++)
#pragma unroll
    for (int c = 0; c < BS; c++) inv[r * BS + c] = m[r][BS + c];
  return ok;
}

__device__ __forceinline__ void unpack_info(int info, int& lfirst, int& dslot, int& ulast, int& lf,
                                            int& lb) {
  lfirst = info & 15; dslot = (info >> 4) & 15; ulast = (info >> 8) & 15;
  lf = (info >> 12) & 1023; lb = (info >> 22) & 1023;
}

// descriptor of the launch-per-level path (subdomains of any size, rows of any width: ILU(k) fill): 8-bit slots
__device__ __forceinline__ void unpack_info_wide(int info, int& lfirst, int& dslot, int& ulast) {
  lfirst = info & 255; dslot = (info >> 8) & 255; ulast = (info >> 16) & 255;
}

// descriptor of the brick schedules with rows of 9 .. 16 blocks (IluSchedule::row_infow: k_ilu_factor_wide, k_pc_wide):
// low word lfirst | dslot << 5 | ulast << 10, high word lev_f | lev_b << 10
__device__ __forceinline__ void unpack_info_w(unsigned long long info, int& lfirst, int& dslot, int& ulast, int& lf,
                                              int& lb) {
  const unsigned w0 = (unsigned)info, w1 = (unsigned)(info >> 32);
  lfirst = w0 & 31; dslot = (w0 >> 5) & 31; ulast = (w0 >> 10) & 31;
  lf = w1 & 1023; lb = (w1 >> 10) & 1023;
}

}  // namespace wai
