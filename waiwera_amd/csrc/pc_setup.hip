// Preconditioner set-up of libwaiwera_hip.so: the symbolic phase of block-Jacobi ILU(0) on the brick subdomains
// (dependency levels, kernel selection), the extended systems of PCASM and ILU(k) (overlapped row sets across rank
// boundaries, level-of-fill patterns), the dense block inverses of PCLU, and the numeric set-up that PCSetUp stands for
// (src/timestepper.F90:1645-1836).
#include "host.hpp"
#include "asm_pattern.hpp"

using namespace wai;

namespace wai {

// The schedule of block-Jacobi ILU(0) on a block matrix given as host CSR (ascending columns), on the device: the options
// from the context, the environment and the build's switches; every fact and table from build_host_schedule
// (ilu_schedule.hpp); the uploads; the factor's own buffers.  `ghosts`: rows may have columns >= n (partition ghosts).
// row_tile (optional; wai_set_pc_tiles): a tile id per row -- a schedule that comes out big (by its row count or its fill, not
// sub lu) gets the tile schedule of tile_schedule.hpp beside its level sets.
int build_schedule(wai_ctx* c, IluSchedule& s, const std::vector<int>& rowptr, const std::vector<int>& colidx,
                   const std::vector<int>& sub, int N, int W, int np, bool ghosts, bool allow_wide, bool sublu, bool fill,
                   const std::vector<int>* row_tile) {
  ScheduleOpts o;
  o.ghosts = ghosts; o.allow_wide = allow_wide; o.sublu = sublu; o.fill = fill;
  o.mesh_W = c->pat.W;
  o.box_faces = c->mesh.n_halo == 0 && W == 7;   // one rank: the split-kernel measurement's lists (wai_bench_kernel 9, 10)
  // (tests: WAI_COL16_MAX_SEG=<n> lowers the limit so that a structured mesh takes the bail-out an unstructured one would)
  if (const char* e = getenv("WAI_COL16_MAX_SEG")) o.max_seg = std::max(1, std::min(8, atoi(e)));
  // the fallback build that drives the GPU tests through the generic kernels (tools/ci_fallback_kernels.sh)
#ifdef WAI_ILU_GENERAL
  o.ilu_general = true;
#endif
#ifdef WAI_PC_ROWS
  o.pc_rows = WAI_PC_ROWS != 0;
#endif
#ifdef WAI_PC_WAVE
  o.pc_wave = WAI_PC_WAVE != 0;
#endif
  HostSchedule h;
  if (int e = build_host_schedule(rowptr, colidx, sub, N, W, np, o, h, c->err)) return e;
  HostTiles t;
  if (row_tile && h.big && !h.sublu)
    if (int e = build_tile_schedule(rowptr, colidx, sub, h.info, *row_tile, N, h.nlev_f, h.nlev_b, t, c->err)) return e;
  // A schedule built again keeps nothing of the one before: every table is reset, also those the new schedule does not have
  // (a table the host did not make is a null buffer -- a mesh that bails out of col16 must not run on, or report, stale
  // tables), and the facts say "no schedule" until every upload has succeeded
  static_cast<ScheduleFacts&>(s) = ScheduleFacts();
  s.tiles.clear();
  auto put = [c](auto& buf, const auto& v) { buf.reset(); return !v.empty() && buf.upload(c, v); };
  if (put(s.sub_ptr, h.sub) || put(s.sub_nlev, h.nlev) || put(s.row_info, h.info) || put(s.row_infow, h.infow) ||
      put(s.row_uoff, h.uoff) || put(s.row_uoffw, h.uoffw) || put(s.row_tslot, h.tslot) || put(s.sub_split, h.split) ||
      put(s.sub_order, h.order) || put(s.sub_int, h.sub_int) || put(s.sub_bnd, h.sub_bnd) || put(s.ord_f, h.ord_f) ||
      put(s.ord_b, h.ord_b) || put(s.col16, h.c16) || put(s.sub_seg, h.seg) || put(s.t_info, h.t_info) ||
      put(s.t_uoff, h.t_uoff) || put(s.t_col16, h.t_c16) || put(s.sub_desc, h.desc) || put(s.pack_tab[0], h.groups[0]) ||
      put(s.pack_tab[1], h.groups[1]) || put(s.pack_tab[2], h.groups[2]))
    return -1;
  if (t.n_tiles > 0) {
    TileTables& d = s.tiles;
    if (put(d.tile_ptr, t.tile_ptr) || put(d.tile_nin, t.tile_nin) || put(d.ord_f, t.ord_f) || put(d.ord_b, t.ord_b) || put(d.row_lev, t.row_lev)) {
      d.clear();
      return -1;
    }
    static_cast<TileFacts&>(d) = std::move(t);
  }
  static_cast<ScheduleFacts&>(s) = std::move(h);
  if (s.fval.alloc(c, ell_size(np, N, W)) || s.dinv.alloc(c, (size_t)np * np * ell_rows(np, N))) return -1;
  return 0;
}

int ensure_halo_dof(wai_ctx* c, int dof) {   // halo buffers wide enough for `dof` doubles per cell
  if (dof <= c->max_dof_buf) return 0;
  c->max_dof_buf = dof;
  return c->d_sendbuf.alloc(c, (size_t)c->send_total * dof) || c->d_recvbuf.alloc(c, (size_t)c->mesh.n_halo * dof) ? -1 : 0;
}

// The structure of the partition-ghost cells' matrix rows, from their owners (collective).  Every cell gets the
// identity (owner rank, owner's local index); the identities of the ghost cells arrive by a halo exchange, and a
// second exchange carries, for every cell a rank sends, the identities of its row's columns.  The receiver keeps
// the columns it knows (its owned and ghost cells -- what the overlapped row sets can contain) in ascending local
// order, with the sender's slot each came from.
int ghost_rows(wai_ctx* c, const LinSys& sys, std::vector<int>& grp, std::vector<int>& gci, std::vector<int>& gslot) {
  const Pattern& J = c->pat;
  const int N = J.n, H = c->mesh.n_halo, W = J.W;
  std::vector<double> ids((size_t)N + H, -1.0);
  const double base = (double)c->comm->rank * 4294967296.0;
  for (int i = 0; i < N; i++) ids[i] = base + i;
  double* scratch = sys.kv->tmp;   // a Krylov work vector (at least n_prim + 16 doubles): idle while the preconditioner is set up
  HIPCHK(c, hipMemcpyAsync(scratch, ids.data(), sizeof(double) * (N + H), hipMemcpyHostToDevice, c->stream));
  if (halo_exchange(c, scratch, 1)) return -1;
  HIPCHK(c, hipMemcpyAsync(ids.data(), scratch, sizeof(double) * (N + H), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (ensure_halo_dof(c, W * sys.A.bs * sys.A.bs)) return -1;
  std::vector<int> sidx((size_t)c->send_total);
  HIPCHK(c, hipMemcpy(sidx.data(), c->d_send_idx, sizeof(int) * sidx.size(), hipMemcpyDeviceToHost));
  std::vector<double> sb((size_t)c->send_total * W, -1.0), rb((size_t)H * W, -1.0);
  for (int p = 0; p < c->send_total; p++) {
    const int i = sidx[p];
    for (int q = J.h_rowptr[i]; q < J.h_rowptr[i + 1]; q++) sb[(size_t)p * W + (q - J.h_rowptr[i])] = ids[J.h_colidx[q]];
  }
  HIPCHK(c, hipMemcpyAsync(c->d_sendbuf, sb.data(), sizeof(double) * sb.size(), hipMemcpyHostToDevice, c->stream));
  if (comm_exchange(c->comm, c->n_nbr, c->nbr_rank.data(), c->send_ptr.data(), c->recv_ptr.data(), W, c->d_sendbuf, c->d_recvbuf,
                    c->stream, c->err))
    return -1;
  HIPCHK(c, hipMemcpyAsync(rb.data(), c->d_recvbuf, sizeof(double) * rb.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<std::pair<double, int>> known((size_t)N + H);
  for (int i = 0; i < N + H; i++) known[i] = {ids[i], i};
  std::sort(known.begin(), known.end());
  grp.assign((size_t)H + 1, 0);
  gci.clear(); gslot.clear();
  std::vector<std::pair<int, int>> row;
  for (int h = 0; h < H; h++) {
    row.clear();
    for (int q = 0; q < W; q++) {
      const double id = rb[(size_t)h * W + q];
      if (id < 0.0) continue;
      auto it = std::lower_bound(known.begin(), known.end(), std::make_pair(id, -1));
      if (it != known.end() && it->first == id) row.push_back({it->second, q});
    }
    std::sort(row.begin(), row.end());
    for (auto& e : row) { gci.push_back(e.first); gslot.push_back(e.second); }
    grp[h + 1] = (int)gci.size();
  }
  return 0;
}

// Does the extended system of `sys` ask for a fused launch (AsmSystem::fuse_asked)?  The flow system alone, on a mesh of at
// most 8 blocks per row, on one rank, without the source network's blocks in the factor and without sub lu; and
// - block-Jacobi ILU(k), k > 0 (no overlap), unless WAI_ILUK_LEVEL_PATH keeps the launch-per-level path.  Several ranks
//   keep it too: the extended system's schedule carries no interior / face lists for the overlapped halo exchange;
// - PCASM (an overlap, any k >= 0): the extended system's rows are then not the system's own, and k_pc_wide's two-pattern
//   form reads the operator through AsmSystem::ext_row (k_pc_wide<.., MAP>).  Several ranks keep today's launches: the
//   overlap's ghost rows need (A x) two layers deep.  WAI_ASM_UNFUSED=1 keeps them everywhere (the tests' comparison, and
//   the way back).
static bool fuse_wanted(const wai_ctx* c, const LinSys& sys, int overlap, int levels, bool with_net, bool sublu) {
  if (with_net || sublu || &sys != &c->flow || sys.A.dg || c->pat.W > 8 || (c->comm && c->comm->nranks > 1)) return false;
  return overlap > 0 ? levels >= 0 && !c->env.asm_unfused : overlap == 0 && levels > 0 && !c->env.iluk_level_path;
}

// The extended system of PCASM / ILU(k) / sub-preconditioner lu on `sys`: the ghost cells' rows (collective), the pattern
// (build_asm_pattern, asm_pattern.hpp), its uploads, E's schedule and the fusing flags.
// sublu: complete fill instead (sub-preconditioner lu; levels is 0 then)
int build_asm(wai_ctx* c, LinSys& sys, int overlap, int levels, bool with_net, bool sublu) {
  AsmSystem& a = sys.as;
  a = AsmSystem();
  const Pattern& J = c->pat;
  const int N = J.n, np = sys.A.bs;
  // Overlap across rank boundaries (the reference's PCASM subdomains are the ranks and MatIncreaseOverlap
  // pulls in the neighbours' rows): the overlapped sets may contain partition-ghost cells, whose matrix rows come
  // from their owners.  One ghost layer exists, so overlap 1 -- the reference's default -- is exact; a deeper overlap would
  // silently stop at that layer on a rank boundary and is refused instead.
  const bool cross = overlap > 0 && c->comm && c->comm->nranks > 1 && c->mesh.n_halo > 0 && c->n_nbr > 0;
  if (cross && overlap > 1) {
    c->err = "preconditioner asm: overlap > 1 across ranks is not supported (the partition carries one ghost layer); use overlap 1";
    return -2;
  }
  const int H = cross ? c->mesh.n_halo : 0;
  std::vector<int> grp, gci, gslot;
  if (cross && ghost_rows(c, sys, grp, gci, gslot)) return -1;
  AsmPattern p;
  if (int e = build_asm_pattern(J.h_rowptr, J.h_colidx, N, grp, gci, gslot, c->ilu.sub, overlap, levels, sublu,
                                with_net ? c->net.cp_cells : std::vector<int>(), p, c->err))
    return e;
  const int n_ext = (int)p.ext_rows.size(), W = p.W;
  a.n_ext = n_ext;
  a.E.n = n_ext; a.E.ncols = n_ext; a.E.bs = np; a.E.W = W; a.E.nnzb = (int)p.ecol.size();
  if (a.E_col.upload(c, p.ell_col) || a.gmap.upload(c, p.gmap) || a.ext_row.upload(c, p.ext_row) ||
      a.E_val.alloc(c, ell_size(np, n_ext, W)) || a.r_ext.alloc(c, (size_t)np * n_ext + 16))
    return -1;
  a.E.col = a.E_col; a.E.val = a.E_val;
  a.n_net = (int)p.net_pos.size();
  if (a.n_net && (a.net_pos.upload(c, p.net_pos) || a.net_pair.upload(c, p.net_pair))) return -1;
  if (cross && (a.hval.alloc(c, ell_size(np, H, J.W)) || a.r_full.alloc_zeroed(c, (size_t)np * (N + H) + 16))) return -1;
  // (`fill` of build_schedule: the factor has column planes of its own -- ILU(k)'s filled rows, or PCASM's extended blocks)
  const bool fuse = fuse_wanted(c, sys, overlap, levels, with_net, sublu) && !cross;
  // tiles (wai_set_pc_tiles): a row of E inherits the tile of the row it stands for; with ghost rows from other ranks in E
  // (cross) the level path stays
  std::vector<int> etile;
  if (!c->pc_tiles.empty() && !cross && !sublu) {
    const std::vector<int> id = tile_of_rows(c->pc_tiles, N);
    etile.resize(n_ext);
    for (int q = 0; q < n_ext; q++) etile[q] = id[p.ext_rows[q]];
  }
  if (int e = build_schedule(c, a.sched, p.erp, p.ecol, p.ext_ptr, n_ext, W, np, false, levels == 0 || fuse, sublu, fuse,
                             etile.empty() ? nullptr : &etile))
    return e;
  a.fuse_asked = fuse;
  a.fused = fuse && a.sched.wide && (overlap > 0 || n_ext == N);   // (no overlap: E's rows are the system's own, in order)
  a.with_net = with_net;
  a.cross = cross;
  a.overlap = overlap;
  a.levels = levels;
  a.sublu = sublu;
  return 0;
}

// PCLU: dense inverse of every preconditioner block (one block per rank with sub_ptr = NULL), by
// Gauss-Jordan elimination with partial pivoting on the host.  Meant for small systems.
int lu_setup(wai_ctx* c, const LinSys& sys) {
  const Pattern& J = c->pat;
  const int bs = sys.A.bs, bb = bs * bs, nsub = c->ilu.nsub;
  const std::vector<int>& sub = c->ilu.sub;
  LuBlocks& L = c->lu;
  if (L.h_inv_ptr.empty() || L.bs != bs) {   // (laid out per block size: the flow's blocks and a tracer's scalars differ)
    L.bs = 0;
    L.h_inv_ptr.assign((size_t)nsub + 1, 0);
    for (int s = 0; s < nsub; s++) {
      const size_t m = (size_t)(sub[s + 1] - sub[s]) * bs;
      if (m > 8192) { c->err = "preconditioner lu: a block has more than 8192 unknowns (dense inverses; use ilu)"; return -2; }
      L.h_inv_ptr[s + 1] = L.h_inv_ptr[s] + m * m;
    }
    L.total = L.h_inv_ptr[nsub];
    if (L.total > ((size_t)1 << 29)) { c->err = "preconditioner lu: more than 4 GB of dense block inverses"; return -2; }
    if (L.inv.alloc(c, L.total) || L.inv_ptr.upload(c, L.h_inv_ptr)) return -1;
    L.bs = bs;
  }
  std::vector<double> val((size_t)J.nnzb * bb), inv(L.total), A;
  {
    DevBuf<double> tmp;
    if (tmp.alloc(c, val.size())) return -1;
    launch_ell_to_bcsr(c, sys.A, tmp);
    HIPCHK(c, hipMemcpyAsync(val.data(), tmp, val.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  for (int s = 0; s < nsub; s++) {
    const int lo = sub[s], hi = sub[s + 1], m = (hi - lo) * bs;
    A.assign((size_t)m * m, 0.0);
    double* B = inv.data() + L.h_inv_ptr[s];
    std::fill(B, B + (size_t)m * m, 0.0);
    for (int i = 0; i < m; i++) B[(size_t)i * m + i] = 1.0;
    for (int i = lo; i < hi; i++)
      for (int q = J.h_rowptr[i]; q < J.h_rowptr[i + 1]; q++) {
        const int j = J.h_colidx[q];
        if (j < lo || j >= hi) continue;   // couplings leaving the block are dropped (block Jacobi)
        for (int r = 0; r < bs; r++)
          for (int k = 0; k < bs; k++) A[(size_t)((i - lo) * bs + r) * m + (j - lo) * bs + k] = val[(size_t)q * bb + r * bs + k];
      }
    for (int p = 0; p < m; p++) {   // Gauss-Jordan with partial pivoting on [A | B]
      int piv = p;
      for (int r = p + 1; r < m; r++) if (std::fabs(A[(size_t)r * m + p]) > std::fabs(A[(size_t)piv * m + p])) piv = r;
      if (A[(size_t)piv * m + p] == 0.0) return 1;   // singular block: recoverable (KSP_DIVERGED_PC_FAILED)
      if (piv != p)
        for (int k = 0; k < m; k++) { std::swap(A[(size_t)p * m + k], A[(size_t)piv * m + k]); std::swap(B[(size_t)p * m + k], B[(size_t)piv * m + k]); }
      const double d = 1.0 / A[(size_t)p * m + p];
      for (int k = 0; k < m; k++) { A[(size_t)p * m + k] *= d; B[(size_t)p * m + k] *= d; }
      for (int r = 0; r < m; r++) {
        const double f = A[(size_t)r * m + p];
        if (r == p || f == 0.0) continue;
        for (int k = 0; k < m; k++) { A[(size_t)r * m + k] -= f * A[(size_t)p * m + k]; B[(size_t)r * m + k] -= f * B[(size_t)p * m + k]; }
      }
    }
  }
  HIPCHK(c, hipMemcpyAsync(L.inv, inv.data(), L.total * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// The multicolour ordering's symbolic phase on the device (wai_set_pc_ordering): every fact and table from build_colour_order
// (colour_order.hpp) on the mesh's pattern and the subdomains in force, uploaded.  Neither changes after wai_ctx_create, so the
// tables are built once, by the first set-up that needs them.  The factor goes to wai_ctx::ilu's buffers.
static int build_colour(wai_ctx* c) {
  ColourSchedule& k = c->colour;
  if (k.built) return 0;
  const Pattern& J = c->pat;
  HostColourOrder h;
  if (int e = build_colour_order(J.h_rowptr, J.h_colidx, c->ilu.sub, J.n, h, c->err)) return e;
  if (k.sub_ptr.upload(c, h.sub) || k.sub_ncol.upload(c, h.ncolours) || k.rows.upload(c, h.rows) || k.slots.upload(c, h.slots) ||
      k.counts.upload(c, h.counts))
    return -1;
  static_cast<ColourFacts&>(k) = std::move(h);
  k.built = true;
  return 0;
}

// what the multicolour ordering does not combine with, on the flow system under block Jacobi or PCASM: -2 with a text that
// names the setting and what it met
static int colour_refusal(wai_ctx* c, const LinSys& sys, const PcOpts& pc) {
  const char* met = nullptr;
  if (pc.type == WAI_PC_ASM) met = "preconditioner asm (WAI_PC_ASM)";
  else if (pc_sub_lu(pc)) met = "sub-preconditioner lu (WAI_SUB_LU)";
  else if (pc.ilu_levels > 0) met = "ilu_levels > 0 (ILU(k) fill)";
  else if (pc_with_net(c, sys)) met = "source-network blocks in the factor's pattern (wai_set_network_couplings)";
  if (!met) return 0;
  c->err = std::string("wai_set_pc_ordering: the multicolour ordering (WAI_PC_ORDER_MULTICOLOUR) serves bjacobi with ILU(0) alone; it met ") + met;
  return -2;
}

// What the coarse level (wai_set_pc_coarse) does not combine with, from the settings alone -- so every caller decides alike,
// wai_set_pc_coarse when it is asked and the set-up for what was set since: null, or the party it met
const char* coarse_refusal(const wai_ctx* c, bool at_setup) {
  if (c->comm && c->comm->nranks > 1) return "more than one rank";
  if (at_setup ? net_in_operator(c, c->flow) : (c->net.on && c->net.coupling))
    return "source-network couplings in the operator (wai_set_network_couplings)";
  if (c->opts.pc_type == WAI_PC_NONE) return "preconditioner none (WAI_PC_NONE)";
  if (c->opts.pc_type == WAI_PC_LU) return "preconditioner lu (WAI_PC_LU)";
  if (c->pc_ordering == WAI_PC_ORDER_MULTICOLOUR) return "the multicolour ordering (WAI_PC_ORDER_MULTICOLOUR)";
  if (c->tr.nt > 0) return "auxiliary (tracer) systems (wai_set_tracers)";
  return nullptr;
}

// The coarse level's lists on the device (c->coarse.h: build_coarse_space), its matrices and its work vectors
int coarse_upload(wai_ctx* c) {
  CoarseLevel& k = c->coarse;
  const CoarseSpace& h = k.h;
  k.m = h.nc * h.bs;
  k.nblk = (int)h.c_colidx.size();
  std::vector<int> blk_row(k.nblk);
  for (int I = 0; I < h.nc; I++)
    for (int b = h.c_rowptr[I]; b < h.c_rowptr[I + 1]; b++) blk_row[b] = I;
  if (k.agg.upload(c, h.agg) || k.agg_ptr.upload(c, h.agg_ptr) || k.agg_rows.upload(c, h.agg_rows) || k.blk_row.upload(c, blk_row) ||
      k.blk_col.upload(c, h.c_colidx) || k.ent_ptr.upload(c, h.ent_ptr) || k.ent_row.upload(c, h.ent_row) ||
      k.ent_slot.upload(c, h.ent_slot))
    return -1;
  const size_t mm = (size_t)k.m * k.m;
  if (k.Ac.alloc_zeroed(c, mm) || k.W.alloc_zeroed(c, mm) || k.Ainv.alloc_zeroed(c, mm) || k.prow.alloc_zeroed(c, k.m) ||
      k.pcol.alloc_zeroed(c, k.m) || k.perm.alloc_zeroed(c, k.m) || k.src.alloc_zeroed(c, k.m) || k.rc.alloc_zeroed(c, k.m) ||
      k.yc.alloc_zeroed(c, k.m) || k.t.alloc_zeroed(c, (size_t)c->flow.nl + 16) || k.w.alloc_zeroed(c, (size_t)c->flow.nl + 16))
    return -1;
  return 0;
}

// the coarse level's numeric set-up on the values in force: Ac = P^T A P, then its inverse (a zero pivot raises d_flags[0],
// which do_pc_setup reads once for both levels).  The two parts are timed apart while profiling is on
static int coarse_numeric(wai_ctx* c, const LinSys& sys) {
  CoarseLevel& k = c->coarse;
  k.ms_galerkin = k.ms_inverse = 0.f;   // (what an unprofiled set-up reports: WAI_COARSE_TIMES)
  auto timed = [&](float& ms, auto&& run) -> int {
    if (c->prof_on) (void)hipEventRecord(c->pev0, c->stream);
    const int e = run();
    if (c->prof_on) {
      (void)hipEventRecord(c->pev1, c->stream);
      (void)hipEventSynchronize(c->pev1);
      (void)hipEventElapsedTime(&ms, c->pev0, c->pev1);
      c->prof_ms[KC_PC_SETUP] += ms;
      c->prof_n[KC_PC_SETUP] += 1;
    }
    return e;
  };
  if (timed(k.ms_galerkin, [&] { return launch_coarse_galerkin(c, sys.A, k); })) return -1;
  return timed(k.ms_inverse, [&] { return launch_coarse_invert(c, k); });
}

// Sets the preconditioner up for `sys` and records it as the owner of the (shared) factor: 0 done, 1 a pivot failed
// (recoverable; the record stands as it did for the flags read back last), < 0 error
int do_pc_setup(wai_ctx* c, LinSys& sys) {
  read_env(c);
  const PcOpts pc = pc_of(c, sys);   // the system's own choice, or the flow solver's
  if (pc_coarse(c, sys)) {
    if (const char* met = coarse_refusal(c, true)) {
      c->err = std::string("wai_set_pc_coarse: the coarse level serves the flow system under bjacobi or asm on one rank; it met ") + met;
      return -2;
    }
  }
  if (pc.type == WAI_PC_NONE) { c->ilu.owner = &sys; return 0; }
  if (pc.type == WAI_PC_LU) {
    Prof p(c, KC_PC_SETUP);
    const int e = lu_setup(c, sys);
    c->ilu.owner = e == 0 ? &sys : nullptr;
    return e;
  }
  {
    Prof p(c, KC_PC_SETUP);
    const Bcsr& A = sys.A;
    if (c->pc_ordering == WAI_PC_ORDER_MULTICOLOUR && &sys == &c->flow) {
      // the flow system's factor in multicolour order: refusals first, then the symbolic phase (once), then a launch per colour
      if (int e = colour_refusal(c, sys, pc)) return e;
      if (int e = build_colour(c)) return e == -2 ? -2 : -1;
      c->colour.fused = pc_colour_serves(c, A, c->colour, !(c->comm && c->comm->nranks > 1));
      if (launch_colour_factor(c, A, c->colour, c->ilu)) return -1;
    } else if (pc_extended(c, sys)) {
      AsmSystem& as = sys.as;
      const int ov = pc.type == WAI_PC_ASM ? (pc.asm_overlap > 0 ? pc.asm_overlap : 1) : 0;
      const bool sl = pc_sub_lu(pc);
      const int lv = sl ? 0 : std::max(pc.ilu_levels, 0);   // (ilu_levels is ignored under sub-preconditioner lu)
      const bool wn = pc_with_net(c, sys);
      if (as.overlap != ov || as.levels != lv || as.sublu != sl || as.E.bs != A.bs || as.with_net != wn ||
          as.fuse_asked != fuse_wanted(c, sys, ov, lv, wn, sl)) {
        // (a refusal of sub-preconditioner lu is the caller's to read: -2 with its text)
        if (int e = build_asm(c, sys, ov, lv, wn, sl)) return sl && e == -2 ? -2 : (e < 0 ? -1 : e);
      }
      if (as.cross) {   // the ghost cells' matrix rows, from their owners
        const int dof = A.W * A.bs * A.bs;
        if (ensure_halo_dof(c, dof)) return -1;
        launch_pack_rows(c, A);
        if (comm_exchange(c->comm, c->n_nbr, c->nbr_rank.data(), c->send_ptr.data(), c->recv_ptr.data(), dof, c->d_sendbuf,
                          c->d_recvbuf, c->stream, c->err))
          return -1;
        launch_unpack_rows(c, A, as);
      }
      launch_asm_gather_matrix(c, A, as);
      if (launch_ilu_factor_on(c, as.E, as.sched)) return -1;
    } else if (launch_ilu_factor_on(c, A, c->ilu)) return -1;
  }
  if (pc_coarse(c, sys) && coarse_numeric(c, sys)) return -1;
  // The factor buffers are overwritten either way, so whoever owned them owns them no longer; `sys` owns them only when
  // every pivot inverted.  After a failed pivot the next solve, application or measurement sets up again and reports it.
  c->ilu.owner = nullptr;
  int fl[4];
  if (fetch_flags(c, fl)) return -1;
  if (fl[0]) return 1;
  c->ilu.owner = &sys;
  return 0;
}

}  // namespace wai
