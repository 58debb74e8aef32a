// The symbolic phase of block-Jacobi ILU(0) on a block matrix given as host CSR (ascending columns): per-row slot ranges
// inside the row's subdomain, dependency levels of both substitutions, whether ILU(0) ever touches an off-diagonal block
// (if not it is DILU and the fused kernels apply), the compact / parked kernel conditions -- or, for subdomains of more
// than 1024 rows, the level sets of the launch-per-level path.  Pure host code -- no device header, no context, no
// environment -- so that a plain C++ program can call it (tests/pc_setup_host); build_schedule (pc_setup.hip) fills the
// options and uploads what build_host_schedule makes.  Not part of the ABI.
#pragma once
#include <algorithm>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

namespace wai {

// What a schedule says besides its tables: IluSchedule (context.hpp) is these facts plus the tables on the device.
struct ScheduleFacts {
  int nsub = 0, max_rows = 0, max_lev = 0;
  std::vector<int> sub;     // host copy of sub_ptr: nsub + 1 row ranges
  // rows of 9 .. 16 blocks in subdomains of <= 1024 rows (cells with up to 16 faces): k_ilu_factor_wide and k_pc_wide read
  // the 64-bit descriptor, lfirst | dslot<<5 | ulast<<10 in the low word, lev_f | lev_b<<10 in the high one
  bool wide = false;
  bool diag_only = false;   // ILU(0) touches no off-diagonal block in any subdomain (== DILU)
  bool scaled = true;       // diag_only: rows pre-scaled by the inverted pivots
  bool park = true;         // k_pc_park: upper blocks parked in LDS
  int max_nl = 0;           // most in-subdomain lower couplings of any row
  int n_int = 0, n_bnd = 0; // subdomains without / with a partition-ghost column
  int max_ublocks = 0;      // most in-subdomain upper blocks of any subdomain, at most 3 counted per row ...
  int max_ublocks_w = 0;    // ... and all (<= 4) uppers counted
  bool fast3 = false;       // <= 3 lower and <= 3 upper in-subdomain couplings per row, offsets < 4
  int max_nlu = 0;          // most lower or upper in-subdomain couplings of any row
  bool rows_kernel = false; // k_pc_rows (one thread per scalar row) applies and is selected
  bool wave_kernel = false; // k_pc_wave (one wave per brick of <= 64 block rows) applies and is selected
  int n_templates = 0, template_rows = 0;   // shared brick descriptors (t_info, t_uoff, t_c16): 0 without col16
  // short bricks packed into shared k_pc_park workgroups (phase 10), per launch list -- 0 all subdomains, 1 sub_int, 2 sub_bnd:
  // workgroups of the packed launch (0: nothing packs, no table) and bricks that share theirs
  int n_groups[3] = {0, 0, 0}, n_shared[3] = {0, 0, 0};
  // subdomains of more than 1024 rows ("one block per rank", sub_ptr = NULL, is the reference's
  // PCBJACOBI / PCASM default): rows of equal dependency level are independent across all
  // subdomains, so the factorisation and the two substitutions run as one launch per level over
  // the rows of that level (stored factor, unfused)
  bool big = false;
  // sub-preconditioner lu (wai_set_sub_pc): the pattern carries the complete fill of every block -- one row per dependency
  // level -- and k_sublu_factor / k_sublu_solve (pc_lu.hip.h) serve it: one workgroup per block, rows in order.  Such a
  // schedule is `big` as well (8-bit slot descriptors) but has no level sets
  bool sublu = false;
  int nlev_f = 0, nlev_b = 0;
  std::vector<int> lev_f_ptr, lev_b_ptr;   // row ranges of each level in ord_f / ord_b
};

// The facts and every table as the device gets it; an empty vector: the schedule has no such table (a null buffer).
struct HostSchedule : ScheduleFacts {
  std::vector<int> nlev;     // per subdomain: forward levels | backward levels << 16
  std::vector<int> info;     // per row: lfirst | dslot<<4 | ulast<<8 | lev_f<<12 | lev_b<<22 (big, wide: lfirst | dslot<<8 | ulast<<16)
  std::vector<unsigned long long> infow;   // wide: the 64-bit descriptor
  std::vector<int> uoff;     // first parked upper block of a row inside its subdomain (min(uppers, 3) counted per row)
  std::vector<int> uoffw;    // ... all uppers counted
  std::vector<int> tslot;    // per row: slot of A_ki in row k for each of its (<= 4) in-subdomain lower couplings k, 4 bits each (15: none)
  std::vector<int> split;    // per subdomain: leading rows longer than half the block-ELL width (k_pc_rows: MINC bricks)
  std::vector<int> order;    // launch order of all subdomains when they differ in cost
  std::vector<int> sub_int, sub_bnd;   // subdomains none of whose rows has a partition-ghost column, and the others
  std::vector<int> ord_f, ord_b;       // rows sorted by forward level, by backward level
  std::vector<unsigned short> c16;     // [n][8] brick-local 16-bit column indices: segment << 13 | offset
  std::vector<int> seg;                // [nsub][8] first column of each segment
  std::vector<int> t_info, t_uoff;     // [template rows] one copy of identical brick descriptors
  std::vector<unsigned short> t_c16;   // [template rows][8]
  std::vector<int> desc;               // [nsub] first row of the brick's template
  std::vector<int> ucount;             // [nsub] parked upper blocks of the brick (min(uppers, 3) counted per row): max_ublocks is their maximum
  std::vector<int> groups[3];          // per launch list: [n_groups][8 waves][4] brick (-1: none), thread offset, park base, group levels
};

// What build_host_schedule is told besides the pattern.
struct ScheduleOpts {
  bool ghosts = false;       // rows may have columns >= N (partition ghosts): make the interior / face lists
  bool allow_wide = true, sublu = false, fill = false;   // (phase 2, schedule_descriptors)
  int mesh_W = 0;            // most blocks of a row of the mesh's own pattern
  bool box_faces = false;    // take every face of the box for a partition boundary (phase 4)
  int max_seg = 8;           // most col16 segments of a brick, 1 .. 8
  // the switches of the fallback build (tools/ci_fallback_kernels.sh)
  bool ilu_general = false;  // stored L / U factor everywhere
  int pc_rows = -1;          // k_pc_rows forced off (0) or on (1) where it applies; -1: block sizes 3 and 4
  bool pc_wave = true;       // false: without k_pc_wave
};

// the CSR pattern the phases read, and what phase 1 leaves for the later ones
struct ScheduleCsr {
  const std::vector<int>& rowptr;
  const std::vector<int>& colidx;
  const int* row(int i) const { return colidx.data() + rowptr[i]; }
  int count(int i) const { return rowptr[i + 1] - rowptr[i]; }
};
struct ScheduleRows {
  std::vector<int> diag, lfirst, ulast, levf, levb;   // per row: slots of the diagonal, of the subdomain's range; levels
  int max_nu = 0, nlf_all = 0, nlb_all = 0;
  bool offdiag_fill = false;
};

// Does k_pc_park serve a matrix of bs x bs blocks on this schedule?  (Neither big nor wide -- diag_only says so -- hence
// rows of <= 8 blocks; <= 512 rows: a workgroup of <= 512 threads.)  The rule of pc_kernel_kind (kernels_fused.hip) once
// the wide, wave and rows kernels have declined, and of the col16 tables below.
inline bool park_serves(const ScheduleFacts& s, int bs) {
  return bs == 2 && s.park && s.diag_only && s.scaled && s.fast3 && s.max_rows <= 512;
}

// ---- phase 1: slot ranges and levels per subdomain ---------------------------------------------------------------
// rows [lo, hi): the slots that lie in the subdomain and the dependency levels of both substitutions
inline void sub_slots_and_levels(const ScheduleCsr& A, int lo, int hi, ScheduleRows& r, int& nlf, int& nlb) {
  nlf = 0; nlb = 0;
  for (int i = lo; i < hi; i++) {
    const int* row = A.row(i);
    const int cnt = A.count(i);
    int ls = 0;
    while (ls < cnt && row[ls] < lo) ls++;
    int ue = cnt;
    while (ue > 0 && row[ue - 1] >= hi) ue--;
    r.lfirst[i] = ls; r.ulast[i] = ue;
    int lv = 0;
    for (int q = ls; q < r.diag[i]; q++) lv = std::max(lv, r.levf[row[q]] + 1);
    r.levf[i] = lv;
    nlf = std::max(nlf, lv + 1);
  }
  for (int i = hi - 1; i >= lo; i--) {
    const int* row = A.row(i);
    int lv = 0;
    for (int q = r.diag[i] + 1; q < r.ulast[i]; q++) lv = std::max(lv, r.levb[row[q]] + 1);
    r.levb[i] = lv;
    nlb = std::max(nlb, lv + 1);
  }
}

// does the IKJ elimination ever update an off-diagonal block of a row in this subdomain?
inline bool sub_offdiag_fill(const ScheduleCsr& A, int lo, int hi, const ScheduleRows& r) {
  for (int i = lo; i < hi; i++) {
    const int* row = A.row(i);
    for (int q = r.lfirst[i]; q < r.diag[i]; q++) {
      const int k = row[q];
      const int* rk = A.row(k);
      for (int r2 = r.diag[k] + 1; r2 < r.ulast[k]; r2++) {
        const int j = rk[r2];
        if (j == i) continue;
        if (std::binary_search(row + q + 1, row + r.ulast[i], j)) return true;
      }
    }
  }
  return false;
}

// per in-subdomain lower coupling (i, k): the slot of row k that holds A_ki (15: structurally absent), four
// bits each -- the pivot recurrence reads A_ki without chasing row k's descriptor and columns
inline void sub_tslot(const ScheduleCsr& A, int lo, int hi, const ScheduleRows& r, HostSchedule& out) {
  for (int i = lo; i < hi; i++) {
    const int* row = A.row(i);
    int pack = 0;
    for (int q = r.lfirst[i], p = 0; q < r.diag[i] && p < 4; q++, p++) {
      const int k = row[q];
      const int* rk = A.row(k);
      const int* e = std::lower_bound(rk + r.diag[k] + 1, rk + r.ulast[k], i);
      const int r2 = (e < rk + r.ulast[k] && *e == i) ? (int)(e - rk) : 15;
      pack |= (r2 & 15) << (4 * p);
    }
    out.tslot[i] = pack;
    out.max_nl = std::max(out.max_nl, r.diag[i] - r.lfirst[i]);
  }
}

// where a row's parked upper blocks start inside its subdomain, and the extremes the kernel selection asks for
inline void sub_upper_offsets(int lo, int hi, ScheduleRows& r, HostSchedule& out) {
  int ucount = 0, ucountw = 0;
  for (int i = lo; i < hi; i++) {
    const int nL = r.diag[i] - r.lfirst[i], nU = r.ulast[i] - r.diag[i] - 1;
    if (nL > 3 || nU > 3 || r.lfirst[i] > 3 || r.diag[i] > 3) out.fast3 = false;
    out.max_nlu = std::max(out.max_nlu, std::max(nL, nU));
    out.uoff[i] = ucount;
    ucount += std::min(nU, 3);
    out.uoffw[i] = ucountw;
    ucountw += nU;
    r.max_nu = std::max(r.max_nu, nU);
  }
  out.ucount.push_back(ucount);
  out.max_ublocks = std::max(out.max_ublocks, ucount);
  out.max_ublocks_w = std::max(out.max_ublocks_w, ucountw);
}

inline void schedule_rows(const ScheduleCsr& A, int N, ScheduleRows& r, HostSchedule& out) {
  r.diag.resize(N); r.lfirst.resize(N); r.ulast.resize(N); r.levf.resize(N); r.levb.resize(N);
  for (int i = 0; i < N; i++) r.diag[i] = (int)(std::lower_bound(A.row(i), A.row(i) + A.count(i), i) - A.row(i));
  out.nlev.assign(out.nsub, 0);
  out.uoff.assign(N, 0); out.uoffw.assign(N, 0); out.tslot.assign(N, 0);
  out.fast3 = true;
  for (int sd = 0; sd < out.nsub; sd++) {
    const int lo = out.sub[sd], hi = out.sub[sd + 1];
    out.max_rows = std::max(out.max_rows, hi - lo);
    int nlf, nlb;
    sub_slots_and_levels(A, lo, hi, r, nlf, nlb);
    if (!r.offdiag_fill) r.offdiag_fill = sub_offdiag_fill(A, lo, hi, r);
    sub_tslot(A, lo, hi, r, out);
    sub_upper_offsets(lo, hi, r, out);
    out.nlev[sd] = (nlf & 0xffff) | (nlb << 16);
    out.max_lev = std::max(out.max_lev, std::max(nlf, nlb));
    r.nlf_all = std::max(r.nlf_all, nlf); r.nlb_all = std::max(r.nlb_all, nlb);
  }
}

// ---- phase 2: wide / big, the row descriptors --------------------------------------------------------------------
// the brick kernels hold a row's <= 8 blocks in registers and pack slot numbers in 4 bits: wider rows (ILU(k)
// fill) and subdomains of more than 1024 rows take the launch-per-level path, whose descriptor has 8-bit slots.
// A mesh whose own rows are wider (cells with 9 .. 16 faces: mesh_W > 8) has k_pc_wide for its subdomains of <= 1024
// rows of <= 16 blocks: its own Jacobian's and the ILU(0) extended systems of PCASM built on it (`allow_wide`; ILU(k)
// fill stays on the launch-per-level path).  A mesh of at most 8 blocks per row keeps the schedule it always had.
// Sub-preconditioner lu (complete fill: one row per level) has kernels of its own, k_sublu_factor / k_sublu_solve, on
// the 8-bit descriptor and without level sets.
// `fill`: the filled pattern of block-Jacobi ILU(k), k > 0, on a mesh of at most 8 blocks per row (build_asm).  W is the
// filled width -- ILU(1) of a 7-point stencil inside a brick: 13 -- and the wide schedule serves it whatever it is up to
// 16, the factor on this pattern's own column planes and the operator on the Jacobian's (k_pc_wide<.., FILL>).  LDS: one
// solution entry per thread and the reduction scratch must fit the 64 KB a workgroup may ask for (1024 rows of 4 x 4
// blocks: 33 408 bytes); what is left parks upper blocks, rows that do not fit re-read theirs (launch_pc_bs: ucap).
// Wider fill or larger subdomains keep the launch-per-level path.  PCASM's extended system asks the same way (build_asm,
// fuse_wanted: any k >= 0, so W may be 8 or less): blocks that do not fit keep the schedule they always had.
inline int schedule_descriptors(int N, int W, int np, const ScheduleOpts& o, const ScheduleRows& r, HostSchedule& out, std::string& err) {
  out.sublu = o.sublu;
  const size_t lds_fill = ((size_t)(((out.max_rows + 63) / 64) * 64) * np + 80) * sizeof(double);
  out.wide = !o.sublu && o.allow_wide && W <= 16 && out.max_rows <= 1024 &&
             (o.fill ? o.mesh_W <= 8 && lds_fill <= 64 * 1024 && out.max_lev <= 1023 : o.mesh_W > 8 && W > 8);
  out.big = o.sublu || out.max_rows > 1024 || (W > 8 && !out.wide) || (o.fill && !out.wide);
  if (!out.big && out.max_lev > 1023) { err = "more than 1023 dependency levels in a subdomain"; return -2; }
  out.info.resize(N);
  for (int i = 0; i < N; i++)
    out.info[i] = (out.big || out.wide) ? (r.lfirst[i] | (r.diag[i] << 8) | (r.ulast[i] << 16))
                                        : (r.lfirst[i] | (r.diag[i] << 4) | (r.ulast[i] << 8) | (r.levf[i] << 12) | (r.levb[i] << 22));
  if (out.wide) {
    out.infow.resize(N);
    for (int i = 0; i < N; i++)
      out.infow[i] = (unsigned long long)(r.lfirst[i] | (r.diag[i] << 5) | (r.ulast[i] << 10)) |
                     ((unsigned long long)(r.levf[i] | (r.levb[i] << 10)) << 32);
  }
  return 0;
}

// ---- phase 3: launch order ---------------------------------------------------------------------------------------
// Workgroup b of a fused launch runs on XCD b % 8 and takes position (b & 7) * per + (b >> 3) of the
// list it is given, so each XCD works through one contiguous eighth in order.  Where bricks differ in cost (the
// ragged bricks at the upper ends of a rank's box: fewer rows, fewer levels) the long ones go first inside each
// eighth and the short ones last: a launch ends with its shortest workgroups (the tail of 2646 bricks on 768 slots
// at 108^3 is a fifth of the launch).  The eighths themselves stay contiguous -- an XCD's L2 keeps serving the
// neighbour bricks' vector entries.
inline int brick_cost(const HostSchedule& s, int sd) {
  return ((s.nlev[sd] & 0xffff) + (s.nlev[sd] >> 16)) * 4096 + (s.sub[sd + 1] - s.sub[sd]);
}
inline void lpt_order(const HostSchedule& s, std::vector<int>& list) {
  const int n = (int)list.size(), per = (n + 7) >> 3;
  for (int j = 0; j < 8; j++) {
    const int a = std::min(j * per, n), b = std::min((j + 1) * per, n);
    std::stable_sort(list.begin() + a, list.begin() + b, [&](int x, int y) { return brick_cost(s, x) > brick_cost(s, y); });
  }
}
inline void launch_order(HostSchedule& out) {
  if (out.big) return;
  bool uniform = true;
  for (int sd = 1; sd < out.nsub && uniform; sd++) uniform = brick_cost(out, sd) == brick_cost(out, 0);
  if (uniform) return;
  out.order.resize(out.nsub);
  std::iota(out.order.begin(), out.order.end(), 0);
  lpt_order(out, out.order);
}

// ---- phase 4: interior and face lists ----------------------------------------------------------------------------
// subdomains without / with partition-ghost columns (for the overlapped halo exchange); the lists are kept where there
// are subdomains of both kinds
inline void interior_and_face_lists(const ScheduleCsr& A, int N, bool box_faces, HostSchedule& out) {
  std::vector<int> li, lb;
  for (int sd = 0; sd < out.nsub; sd++) {
    bool bnd = false;
    for (int i = out.sub[sd]; i < out.sub[sd + 1] && !bnd; i++) {
      // box_faces, on one rank: for the split-kernel measurement (wai_bench_kernel 9, 10) take the bricks on the
      // faces of the box -- rows with fewer than six neighbours -- as if every face were a partition
      // boundary (what an interior rank of a larger decomposition sees)
      if (box_faces) bnd = A.count(i) < 7;
      else bnd = std::any_of(A.row(i), A.row(i) + A.count(i), [N](int col) { return col >= N; });
    }
    (bnd ? lb : li).push_back(sd);
  }
  out.n_int = (int)li.size();
  out.n_bnd = (int)lb.size();
  lpt_order(out, li); lpt_order(out, lb);
  if (out.n_int > 0 && out.n_bnd > 0) { out.sub_int.swap(li); out.sub_bnd.swap(lb); }
}

// ---- phase 5: level sets -----------------------------------------------------------------------------------------
// level sets over all subdomains: rows of one level are independent wherever they live (wide schedules: for the
// measurement of the launch-per-level path on the same factor, wai_bench_kernel 23)
inline void level_sets(int N, const ScheduleRows& r, HostSchedule& out) {
  out.nlev_f = r.nlf_all; out.nlev_b = r.nlb_all;
  out.ord_f.resize(N); out.ord_b.resize(N);
  out.lev_f_ptr.assign(r.nlf_all + 1, 0); out.lev_b_ptr.assign(r.nlb_all + 1, 0);
  for (int i = 0; i < N; i++) { out.lev_f_ptr[r.levf[i] + 1]++; out.lev_b_ptr[r.levb[i] + 1]++; }
  for (int l = 0; l < r.nlf_all; l++) out.lev_f_ptr[l + 1] += out.lev_f_ptr[l];
  for (int l = 0; l < r.nlb_all; l++) out.lev_b_ptr[l + 1] += out.lev_b_ptr[l];
  std::vector<int> pf(out.lev_f_ptr.begin(), out.lev_f_ptr.end() - 1), pb(out.lev_b_ptr.begin(), out.lev_b_ptr.end() - 1);
  for (int i = 0; i < N; i++) { out.ord_f[pf[r.levf[i]]++] = i; out.ord_b[pb[r.levb[i]]++] = i; }
}

// ---- phase 6: kernel selection -----------------------------------------------------------------------------------
// The switches.  Build time, for the fallback build that drives the GPU tests through the generic kernels
// (tools/ci_fallback_kernels.sh): ScheduleOpts::ilu_general, pc_rows, pc_wave.  Run time, for the tests that compare paths
// in one process: WAI_NO_COL16 (k_pc_park on the int32 column planes: read_env) and ScheduleOpts::max_seg.
inline void select_kernels(int W, int np, const ScheduleOpts& o, const ScheduleRows& r, HostSchedule& out) {
  out.diag_only = !r.offdiag_fill && !out.big && !out.wide;   // (wide rows: the stored factor alone, k_pc_wide)
  out.scaled = true;
  if (o.ilu_general) out.diag_only = false;
  // 160 KB of LDS per CU; a workgroup may use 64 KB
  const size_t need = ((size_t)(((out.max_rows + 63) / 64) * 64) * np + 32 + (size_t)out.max_ublocks * 4) * sizeof(double);
  out.park = need <= 64 * 1024;
  // one thread per scalar row: needs the pivot-scaled DILU form, <= 4 + 4 couplings and a brick whose
  // scalar rows fit one workgroup.  Default for block sizes 3 and 4, where a whole block row per
  // thread does not fit the register file (pc_rows 0 / 1 forces it off / on, bs <= 2 too).
  const bool can = out.diag_only && out.scaled && !out.big && out.max_nlu <= 4 && out.max_rows * np <= 1024 && W <= 8;
  out.rows_kernel = can && (o.pc_rows < 0 ? np >= 3 : o.pc_rows != 0);
  // one wave per brick: <= 64 block rows, <= 3 lower and <= 4 upper in-brick couplings, LDS for four bricks per
  // workgroup within 64 KB (pc_wave false builds without)
  const size_t lds_w = (size_t)4 * (64 * np + (size_t)out.max_ublocks_w * np * np) * sizeof(double);
  out.wave_kernel = out.rows_kernel && np == 3 && out.max_rows <= 64   // (4 x 4 blocks: 174 VGPRs, two waves per SIMD -- not measured, k_pc_rows keeps them)
                    && out.max_nl <= 3 && r.max_nu <= 4 && lds_w <= 64 * 1024 && o.pc_wave;
}

// ---- phase 7: the rows kernel's split record ---------------------------------------------------------------------
// bricks whose long rows come first (MINC: fracture cells, then their matrix cells with 2 of 8
// slots): k_pc_rows maps the long rows of all components to the first waves, so that a wave is
// all-long or all-short and the short ones skip the slot loop instead of idling in it.  Kept where some brick has such rows
inline void rows_split_record(const ScheduleCsr& A, int W, HostSchedule& out) {
  std::vector<int> split(out.nsub);
  bool any = false;
  for (int sd = 0; sd < out.nsub; sd++) {
    const int lo = out.sub[sd], hi = out.sub[sd + 1];
    int r1 = lo;
    while (r1 < hi && A.count(r1) * 2 > W) r1++;
    bool sorted = true;
    for (int i = r1; i < hi && sorted; i++) sorted = A.count(i) * 2 <= W;
    split[sd] = (sorted && r1 > lo) ? r1 - lo : hi - lo;
    any = any || split[sd] != hi - lo;
    // bits 16+: the most blocks a short row of the brick has, or 15 where short rows are mixed among the long ones.
    // k_pc_wave then knows a row's slot count from the brick's record -- long rows take all W slots (a missing
    // neighbour's padding: a zero block on the own column) -- instead of waiting for rowptr before its first block load
    int short_cnt = 0;
    for (int i = r1; i < hi; i++) short_cnt = std::max(short_cnt, A.count(i));
    bool mixed = false;
    for (int i = lo; i < hi && !mixed; i++) mixed = (i < r1) != (A.count(i) * 2 > W);
    split[sd] |= (mixed || !sorted ? 15 : short_cnt) << 16;
  }
  if (any) out.split.swap(split);
}

// ---- phase 8: 16-bit column indices ------------------------------------------------------------------------------
// k_pc_park's column indices as 16-bit (segment, offset) pairs -- 14 of a row's 304 bytes less per launch.  Segment 0
// starts at the brick's own first row; the others are windows of 8192 columns over what the brick reaches outside itself.
// False, and no table, where some brick needs more than max_seg segments (tests lower the limit so that a structured mesh
// takes the bail-out an unstructured one would).

// one brick's segments into sg[0 .. 8); their number, or 0 where max_seg do not do
inline int brick_segments(const ScheduleCsr& A, int lo, int hi, int max_seg, int* sg, std::vector<int>& far) {
  far.clear();
  for (int i = lo; i < hi; i++)
    for (int q = 0; q < A.count(i); q++)
      if (A.row(i)[q] < lo || A.row(i)[q] >= hi) far.push_back(A.row(i)[q]);
  std::sort(far.begin(), far.end());
  far.erase(std::unique(far.begin(), far.end()), far.end());
  int nseg = 1;
  sg[0] = lo;
  for (size_t k = 0; k < far.size();) {
    if (nseg == max_seg) return 0;
    const int base = far[k];
    sg[nseg++] = base;
    while (k < far.size() && far[k] - base < 8192) k++;
  }
  return nseg;
}
inline bool col16_indices(const ScheduleCsr& A, int N, int W, int max_seg, HostSchedule& out) {
  std::vector<unsigned short> c16((size_t)8 * N, 0);      // [row][8]: a row's indices are ONE 16-byte load
  std::vector<int> seg((size_t)out.nsub * 8, 0);
  std::vector<int> far;
  for (int sd = 0; sd < out.nsub; sd++) {
    const int lo = out.sub[sd], hi = out.sub[sd + 1];
    int* sg = seg.data() + (size_t)sd * 8;
    const int nseg = brick_segments(A, lo, hi, max_seg, sg, far);
    if (nseg == 0) return false;
    for (int i = lo; i < hi; i++)
      for (int q = 0; q < W; q++) {
        const int cg = q < A.count(i) ? A.row(i)[q] : i;      // padding: the own column (a zero block), as Bcsr::col has it
        int sgi = 0;
        if (cg < lo || cg >= hi) {
          sgi = nseg - 1;
          while (sgi > 0 && !(cg >= sg[sgi] && cg - sg[sgi] < 8192)) sgi--;
          if (sgi == 0) return false;
        }
        c16[(size_t)i * 8 + q] = (unsigned short)((sgi << 13) | (cg - sg[sgi]));
      }
  }
  out.c16.swap(c16); out.seg.swap(seg);
  return true;
}

// ---- phase 9: descriptor templates -------------------------------------------------------------------------------
// one copy of identical brick descriptors (IluSchedule::t_*): two bricks share a template when they have the same row
// count and the same row_info, row_uoff and col16 bytes.  Template k is rows [first, first + rows of the brick) of t_*
inline void descriptor_templates(HostSchedule& out) {
  std::unordered_map<std::string, int> seen;   // a brick's descriptor bytes -> first row of its template
  auto bytes = [](const void* p, size_t n) { return std::string(static_cast<const char*>(p), n); };
  out.desc.resize(out.nsub);
  for (int sd = 0; sd < out.nsub; sd++) {
    const int lo = out.sub[sd], R = out.sub[sd + 1] - lo;
    const std::string key = bytes(&R, sizeof(int)) + bytes(out.info.data() + lo, sizeof(int) * R) +
                            bytes(out.uoff.data() + lo, sizeof(int) * R) +
                            bytes(out.c16.data() + (size_t)lo * 8, sizeof(unsigned short) * 8 * R);
    const auto it = seen.emplace(key, (int)out.t_info.size());
    if (it.second) {
      out.n_templates++;
      out.t_info.insert(out.t_info.end(), out.info.begin() + lo, out.info.begin() + lo + R);
      out.t_uoff.insert(out.t_uoff.end(), out.uoff.begin() + lo, out.uoff.begin() + lo + R);
      out.t_c16.insert(out.t_c16.end(), out.c16.begin() + (size_t)lo * 8, out.c16.begin() + (size_t)(lo + R) * 8);
    }
    out.desc[sd] = it.first->second;
  }
  out.template_rows = (int)out.t_info.size();
}

// ---- phase 10: short bricks packed into shared workgroups --------------------------------------------------------
// A k_pc_park workgroup has one thread per row of the LARGEST brick, and a brick's life -- descriptors, indices, seven slot
// round trips, two LDS round trips per level, epilogue -- hardly shortens with fewer rows: a ragged brick at the upper end
// of the box holds its slot nearly as long as a full one (216 = 13 x 16 + 8: 27 of a layer pair's 196 workgroups carry
// 7 % of its rows).  So the short bricks of a launch list share workgroups: a GROUP is 1 .. 8 bricks of one list, each on
// whole waves of its own (thread offsets are multiples of 64: a wave never holds rows of two bricks), together within the
// workgroup's threads and within max_ublocks parked blocks -- the launch's LDS request and the workgroups per CU stay what
// they are.  The bricks, their arithmetic and their partial sums are untouched; only which workgroup, and which of its
// waves, runs a brick changes.  First-fit decreasing over the list's short bricks (ties by brick index); bricks as wide as
// the workgroup stay alone.  A group takes the place of its first member, then the eighths and the longest-first order of
// phase 3 on the group's cost: its largest level counts, then its rows.
// The record of (group, wave), one 16-byte scalar load: the wave's brick or -1, the thread offset of that brick in the
// workgroup, its first block in the park, the group's level counts (forward | backward << 16, each the maximum over the
// members: every wave takes part in every barrier).  A list in which nothing packs has no table and launches as before.
constexpr int PACK_WAVES = 8, PACK_REC = 4;
inline void pack_list(const HostSchedule& s, std::vector<int> list, std::vector<int>& table, int& n_groups, int& n_shared) {
  table.clear(); n_groups = 0; n_shared = 0;
  const int T = ((s.max_rows + 63) / 64) * 64;
  auto rows = [&](int sd) { return s.sub[sd + 1] - s.sub[sd]; };
  auto threads = [&](int sd) { return ((rows(sd) + 63) / 64) * 64; };
  if (T > 64 * PACK_WAVES) return;
  std::sort(list.begin(), list.end());        // the list's natural order: the lists themselves are kept longest-first
  std::vector<int> shorts;
  for (int sd : list) if (threads(sd) < T) shorts.push_back(sd);
  std::stable_sort(shorts.begin(), shorts.end(), [&](int a, int b) { return rows(a) > rows(b); });
  struct Bin { std::vector<int> members; int threads = 0, ublocks = 0; };
  std::vector<Bin> bins;
  std::unordered_map<int, int> opens;         // a bin's first member -> the bin
  bool any = false;
  for (int sd : shorts) {
    size_t b = 0;
    while (b < bins.size() && (bins[b].threads + threads(sd) > T || bins[b].ublocks + s.ucount[sd] > s.max_ublocks)) b++;
    if (b == bins.size()) { bins.emplace_back(); opens[sd] = (int)b; }
    else any = true;
    bins[b].members.push_back(sd); bins[b].threads += threads(sd); bins[b].ublocks += s.ucount[sd];
  }
  if (!any) return;
  std::vector<std::vector<int>> groups;       // in the order of their first members
  for (int sd : list) {
    if (threads(sd) >= T) groups.push_back({sd});
    else if (opens.count(sd)) groups.push_back(bins[opens[sd]].members);
  }
  auto levels = [&](const std::vector<int>& g, int& nlf, int& nlb) {
    nlf = 0; nlb = 0;
    for (int sd : g) { nlf = std::max(nlf, s.nlev[sd] & 0xffff); nlb = std::max(nlb, s.nlev[sd] >> 16); }
  };
  auto cost = [&](const std::vector<int>& g) {
    int nlf, nlb, r = 0;
    levels(g, nlf, nlb);
    for (int sd : g) r += rows(sd);
    return (nlf + nlb) * 4096 + r;
  };
  const int n = (int)groups.size(), per = (n + 7) >> 3;
  for (int j = 0; j < 8; j++) {
    const int a = std::min(j * per, n), b = std::min((j + 1) * per, n);
    std::stable_sort(groups.begin() + a, groups.begin() + b,
                     [&](const std::vector<int>& x, const std::vector<int>& y) { return cost(x) > cost(y); });
  }
  table.assign((size_t)n * PACK_WAVES * PACK_REC, 0);
  for (int g = 0; g < n; g++) {
    int nlf, nlb, toff = 0, ubase = 0;
    levels(groups[g], nlf, nlb);
    int* rec = table.data() + (size_t)g * PACK_WAVES * PACK_REC;
    for (int w = 0; w < PACK_WAVES; w++) { rec[w * PACK_REC] = -1; rec[w * PACK_REC + 1] = w * 64; rec[w * PACK_REC + 3] = nlf | (nlb << 16); }
    for (int sd : groups[g]) {
      for (int w = toff / 64; w < (toff + threads(sd)) / 64; w++) {
        rec[w * PACK_REC] = sd; rec[w * PACK_REC + 1] = toff; rec[w * PACK_REC + 2] = ubase;
      }
      toff += threads(sd); ubase += s.ucount[sd];
    }
    if (groups[g].size() > 1) n_shared += (int)groups[g].size();
  }
  n_groups = n;
}
inline void pack_groups(HostSchedule& out) {
  std::vector<int> all(out.nsub);
  std::iota(all.begin(), all.end(), 0);
  pack_list(out, all, out.groups[0], out.n_groups[0], out.n_shared[0]);
  if (!out.sub_int.empty()) pack_list(out, out.sub_int, out.groups[1], out.n_groups[1], out.n_shared[1]);
  if (!out.sub_bnd.empty()) pack_list(out, out.sub_bnd, out.groups[2], out.n_groups[2], out.n_shared[2]);
}

// The schedule of the N x N block matrix (rowptr, colidx: rows of at most W blocks, of np x np entries each) under the
// subdomains sub[0] = 0 <= .. <= sub[nsub] = N.  Returns 0, or -2 with `err` set; `out` is built from nothing either way.
inline int build_host_schedule(const std::vector<int>& rowptr, const std::vector<int>& colidx, const std::vector<int>& sub,
                               int N, int W, int np, const ScheduleOpts& opts, HostSchedule& out, std::string& err) {
  out = HostSchedule();
  if (sub.empty() || sub.front() != 0 || sub.back() != N) { err = "sub_ptr must cover [0, n_owned]"; return -2; }
  if (!std::is_sorted(sub.begin(), sub.end())) { err = "sub_ptr not monotone"; return -2; }
  out.sub = sub;
  out.nsub = (int)sub.size() - 1;
  const ScheduleCsr A{rowptr, colidx};
  ScheduleRows r;
  schedule_rows(A, N, r, out);
  if (int e = schedule_descriptors(N, W, np, opts, r, out, err)) return e;
  launch_order(out);
  if (opts.ghosts) interior_and_face_lists(A, N, opts.box_faces, out);
  if ((out.big || out.wide) && !opts.sublu) level_sets(N, r, out);
  select_kernels(W, np, opts, r, out);
  if (out.rows_kernel) rows_split_record(A, W, out);
  if (park_serves(out, np) && col16_indices(A, N, W, opts.max_seg, out)) descriptor_templates(out);
  if (park_serves(out, np)) pack_groups(out);
  return 0;
}

}  // namespace wai
