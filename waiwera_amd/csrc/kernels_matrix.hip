// K6 and the matrix copies: block SpMV, the BCSR <-> block-ELL conversion, the halo rows' pack / unpack, the PCASM
// gathers and scatters, and their launchers.
#include "linalg_device.hip.h"

namespace wai {

// ---- K6: block SpMV --------------------------------------------------------------------------
// rowptr (may be null): rows shorter than the block-ELL width (MINC matrix cells: 2 blocks of 8)
// skip their padding slots instead of streaming zeros
template <int BS, bool SHORT, int WM>
__device__ __forceinline__ void spmv_row(int n, int W, int nblk, const int* __restrict__ col,
                                         const double* __restrict__ val, const int* __restrict__ rowptr,
                                         const double* __restrict__ x, double* __restrict__ y) {
  const int b = xcd_remap(blockIdx.x, nblk);
  const int i = b * TPB + threadIdx.x;
  if (b >= nblk || i >= n) return;
  double acc[BS];
#pragma unroll
  for (int r = 0; r < BS; r++) acc[r] = 0.0;
  ell_row_mult<BS, WM>(n, SHORT ? rowptr[i + 1] - rowptr[i] : W, i, col, val, x, acc);
  if constexpr (BS == 2) store_z2(y, (size_t)i, acc[0], acc[1]);
  else if constexpr (BS == 3) {
    double* p = y + (size_t)i * 3;
    wai_d2u t = {acc[0], acc[1]};
    *reinterpret_cast<wai_d2u*>(p) = t;
    p[2] = acc[2];
  }
  else {
#pragma unroll
    for (int r = 0; r < BS; r++) y[(size_t)i * BS + r] = acc[r];
  }
}
template <int BS, bool SHORT>
__global__ __launch_bounds__(TPB) void k_spmv(int n, int W, int nblk, const int* __restrict__ col,
                                              const double* __restrict__ val, const int* __restrict__ rowptr,
                                              const double* __restrict__ x, double* __restrict__ y) {
  spmv_row<BS, SHORT, WMAX>(n, W, nblk, col, val, rowptr, x, y);
}
// Rows of 9 .. 16 blocks (cells with up to 16 faces: polygonal columns, refined grids with hanging nodes).  The same
// slot-at-a-time streaming as k_spmv, sixteen guarded slots instead of eight; such meshes have ragged rows, so the
// launcher takes the rowptr form wherever padding exceeds 10 %.
template <int BS, bool SHORT>
__global__ __launch_bounds__(TPB) void k_spmv_wide(int n, int W, int nblk, const int* __restrict__ col,
                                                   const double* __restrict__ val, const int* __restrict__ rowptr,
                                                   const double* __restrict__ x, double* __restrict__ y) {
  spmv_row<BS, SHORT, WMAX_WIDE>(n, W, nblk, col, val, rowptr, x, y);
}

// ---- layout conversion (C ABI exchanges BCSR) -------------------------------------------------
__global__ __launch_bounds__(TPB) void k_ell_to_bcsr(int n, int W, int bs, const int* __restrict__ rowptr,
                                                     const double* __restrict__ ell, double* __restrict__ bcsr) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= (size_t)n * W) return;
  const int s = (int)(t / n), i = (int)(t - (size_t)s * n);
  const int a = rowptr[i], cnt = rowptr[i + 1] - a, bb = bs * bs;
  if (s >= cnt) return;
  for (int e = 0; e < bb; e++) bcsr[(size_t)(a + s) * bb + e] = ell[ell_ix(bs, (size_t)n, s, e / bs, e % bs, (size_t)i)];
}
__global__ __launch_bounds__(TPB) void k_bcsr_to_ell(int n, int W, int bs, const int* __restrict__ rowptr,
                                                     const double* __restrict__ bcsr, double* __restrict__ ell) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= (size_t)n * W) return;
  const int s = (int)(t / n), i = (int)(t - (size_t)s * n);
  const int a = rowptr[i], cnt = rowptr[i + 1] - a, bb = bs * bs;
  for (int e = 0; e < bb; e++)
    ell[ell_ix(bs, (size_t)n, s, e / bs, e % bs, (size_t)i)] = (s < cnt) ? bcsr[(size_t)(a + s) * bb + e] : 0.0;
}

// ---- PCASM: extended system ---------------------------------------------------------------------
// E.val plane element <- J.val plane element (gmap = slot*n + row of the source block, -1: none)
// gmap: >= 0 slot * n + row of the source block in J; -1 none (zero block); <= -2: -(g + 2) = slot * n_halo + ghost
// cell, a block of a partition-ghost cell's row as received from its owner (hval)
__global__ __launch_bounds__(TPB) void k_asm_gather_matrix(int n, int n_ext, int W_ext, int bs, int n_halo,
                                                           const int* __restrict__ gmap,
                                                           const double* __restrict__ jval,
                                                           const double* __restrict__ hval, double* __restrict__ eval) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= (size_t)W_ext * n_ext) return;
  const int s = (int)(t / n_ext), q = (int)(t - (size_t)s * n_ext);
  const int g = gmap[t];
  const bool ghost = g <= -2;
  const int gg = ghost ? -(g + 2) : g, nn = ghost ? n_halo : n;
  const double* src = ghost ? hval : jval;
  const int ss = g == -1 ? 0 : gg / nn, i = g == -1 ? 0 : gg - ss * nn;
  for (int r = 0; r < bs; r++)
    for (int k = 0; k < bs; k++)
      eval[ell_ix(bs, (size_t)n_ext, s, r, k, (size_t)q)] = g == -1 ? 0.0 : src[ell_ix(bs, (size_t)nn, ss, r, k, (size_t)i)];
}
// the source network's blocks added where the extended pattern holds their pair of cells (AsmSystem::net_pos / net_pair;
// cp: [row][column][bs][bs] row-major, m columns): thread per (entry, r, k)
__global__ __launch_bounds__(TPB) void k_asm_add_couplings(int n_net, int n_ext, int bs, const int* __restrict__ pos,
                                                           const int* __restrict__ pair, const double* __restrict__ cp,
                                                           double* __restrict__ eval) {
  const int t = blockIdx.x * TPB + threadIdx.x, bb = bs * bs;
  if (t >= n_net * bb) return;
  const int e = t / bb, rk = t - e * bb, r = rk / bs, k = rk - r * bs;
  const int sl = pos[e] / n_ext, q = pos[e] - sl * n_ext;
  eval[ell_ix(bs, (size_t)n_ext, sl, r, k, (size_t)q)] += cp[(size_t)pair[e] * bb + rk];
}
// matrix rows of the cells a rank sends to its neighbours: buf[p][slot][r][k] (W * bs * bs doubles per cell)
__global__ __launch_bounds__(TPB) void k_pack_rows(int n, int W, int bs, int nsend, const int* __restrict__ idx,
                                                   const double* __restrict__ jval, double* __restrict__ buf) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  const int bb = bs * bs, dof = W * bb;
  if (t >= (size_t)nsend * dof) return;
  const int p = (int)(t / dof), e = (int)(t - (size_t)p * dof), sl = e / bb, rk = e - sl * bb;
  buf[t] = jval[ell_ix(bs, (size_t)n, sl, rk / bs, rk % bs, (size_t)idx[p])];
}
// ... and on the receiving side into block-ELL planes over the ghost cells (receive buffer in ghost order)
__global__ __launch_bounds__(TPB) void k_unpack_rows(int n_halo, int W, int bs, const double* __restrict__ buf,
                                                     double* __restrict__ hval) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  const int bb = bs * bs, dof = W * bb;
  if (t >= (size_t)n_halo * dof) return;
  const int h = (int)(t / dof), e = (int)(t - (size_t)h * dof), sl = e / bb, rk = e - sl * bb;
  hval[ell_ix(bs, (size_t)n_halo, sl, rk / bs, rk % bs, (size_t)h)] = buf[t];
}
__global__ __launch_bounds__(TPB) void k_asm_gather(int n_ext, int bs, const int* __restrict__ ext_row,
                                                    const double* __restrict__ r, double* __restrict__ r_ext) {
  const int q = blockIdx.x * TPB + threadIdx.x;
  if (q >= n_ext) return;
  const int i = ext_row[q] & 0x7fffffff;
  for (int k = 0; k < bs; k++) r_ext[(size_t)q * bs + k] = r[(size_t)i * bs + k];
}
__global__ __launch_bounds__(TPB) void k_asm_scatter(int n_ext, int bs, const int* __restrict__ ext_row,
                                                     const double* __restrict__ z_ext, double* __restrict__ z) {
  const int q = blockIdx.x * TPB + threadIdx.x;
  if (q >= n_ext) return;
  const int e = ext_row[q];
  if (e >= 0) return;  // overlap row: not prolonged back (PC_ASM_RESTRICT)
  const int i = e & 0x7fffffff;
  for (int k = 0; k < bs; k++) z[(size_t)i * bs + k] = z_ext[(size_t)q * bs + k];
}

int launch_spmv(wai_ctx* c, const Bcsr& J, const double* x, double* y) {
  c->ks.n_launch++;
  if (J.dg) return launch_dg_spmv(c, J, x, y);   // the coupled tracer system
  const int nblk = (J.n + TPB - 1) / TPB;
  const int grid = ((nblk + 7) / 8) * 8;
  const int* rp = (size_t)J.nnzb * 10 < (size_t)J.n * J.W * 9 ? J.rowptr : nullptr;   // > 10 % padding
  if (J.W > WMAX_WIDE) return -1;   // (wai_ctx_create refuses wider rows)
  return with_bs(J.bs, [&](auto bs) {
    with_flag(rp != nullptr, [&](auto sh) {
      constexpr int BS = decltype(bs)::value;
      constexpr bool SHORT = decltype(sh)::value;
      if (J.W > WMAX)   // cells with 9 .. 16 faces
        hipLaunchKernelGGL((k_spmv_wide<BS, SHORT>), grid, TPB, 0, c->stream, J.n, J.W, nblk, J.col, J.val, rp, x, y);
      else
        hipLaunchKernelGGL((k_spmv<BS, SHORT>), grid, TPB, 0, c->stream, J.n, J.W, nblk, J.col, J.val, rp, x, y);
    });
  });
}

int launch_asm_gather_matrix(wai_ctx* c, const Bcsr& J, const AsmSystem& a) {
  const size_t tot = (size_t)a.E.W * a.n_ext;
  hipLaunchKernelGGL(k_asm_gather_matrix, (int)((tot + TPB - 1) / TPB), TPB, 0, c->stream, J.n, a.n_ext, a.E.W,
                     a.E.bs, c->mesh.n_halo, a.gmap, J.val, a.hval, a.E.val);
  if (a.with_net && a.n_net > 0 && c->net.cp_valid && c->net.d_cp_val) {   // + the source network's blocks of this Jacobian
    const int nt = a.n_net * a.E.bs * a.E.bs;
    hipLaunchKernelGGL(k_asm_add_couplings, (nt + TPB - 1) / TPB, TPB, 0, c->stream, a.n_net, a.n_ext, a.E.bs, a.net_pos,
                       a.net_pair, c->net.d_cp_val, a.E.val);
  }
  return 0;
}
int launch_pack_rows(wai_ctx* c, const Bcsr& J) {
  const size_t tot = (size_t)c->send_total * J.W * J.bs * J.bs;
  if (tot) hipLaunchKernelGGL(k_pack_rows, (int)((tot + TPB - 1) / TPB), TPB, 0, c->stream, J.n, J.W, J.bs, c->send_total,
                              c->d_send_idx, J.val, c->d_sendbuf);
  return 0;
}
int launch_unpack_rows(wai_ctx* c, const Bcsr& J, const AsmSystem& a) {
  const size_t tot = (size_t)c->mesh.n_halo * J.W * J.bs * J.bs;
  if (tot) hipLaunchKernelGGL(k_unpack_rows, (int)((tot + TPB - 1) / TPB), TPB, 0, c->stream, c->mesh.n_halo, J.W, J.bs,
                              c->d_recvbuf, a.hval);
  return 0;
}
int launch_asm_gather(wai_ctx* c, const AsmSystem& a, const double* r) {
  hipLaunchKernelGGL(k_asm_gather, (a.n_ext + TPB - 1) / TPB, TPB, 0, c->stream, a.n_ext, a.E.bs, a.ext_row, r, a.r_ext);
  return 0;
}
int launch_asm_scatter(wai_ctx* c, const AsmSystem& a, double* z) {
  hipLaunchKernelGGL(k_asm_scatter, (a.n_ext + TPB - 1) / TPB, TPB, 0, c->stream, a.n_ext, a.E.bs, a.ext_row, a.r_ext, z);
  return 0;
}

int launch_ell_to_bcsr(wai_ctx* c, const Bcsr& J, double* bcsr) {
  const size_t tot = (size_t)J.n * J.W;
  hipLaunchKernelGGL(k_ell_to_bcsr, (int)((tot + TPB - 1) / TPB), TPB, 0, c->stream, J.n, J.W, J.bs, J.rowptr, J.val, bcsr);
  return 0;
}
int launch_bcsr_to_ell(wai_ctx* c, const double* bcsr, const Bcsr& J) {
  const size_t tot = (size_t)J.n * J.W;
  hipLaunchKernelGGL(k_bcsr_to_ell, (int)((tot + TPB - 1) / TPB), TPB, 0, c->stream, J.n, J.W, J.bs, J.rowptr, bcsr, J.val);
  return 0;
}

}  // namespace wai
