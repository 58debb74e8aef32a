// The context of libwaiwera_hip.so behind its C ABI (include/waiwera_hip.h): creation from the mesh, EOS and solver
// descriptions, the solver settings, the halo and the communicator, regions, curve tables, boundary conditions and rock
// updates.  The mesh's connectivity and matrix pattern are built on the host alone (mesh_pattern.hpp) and uploaded here.
#include "host.hpp"
#include "cell_order.hpp"
#include <cstdio>

using namespace wai;

namespace wai {

// a set of Krylov work vectors for vectors of nl entries, zeroed (those it has already are kept)
int alloc_krylov_vecs(wai_ctx* c, KrylovVecs& k, size_t nl) {
  for (auto p : {&k.R, &k.RP, &k.P, &k.V, &k.S, &k.T, &k.tmp, &k.X_own})
    if (!*p && p->alloc_zeroed(c, nl + 16)) return -1;
  k.X = k.X_own;
  return 0;
}
// a GMRES basis of at least m vectors for sys: m + 1 directions, + 2 error approximations + the update (lgmres)
int ensure_basis(wai_ctx* c, LinSys& sys, int m) {
  KrylovVecs& k = *sys.kv;
  if (k.basis && k.basis_m >= m) return 0;
  k.basis_m = m;
  return k.basis.alloc_zeroed(c, (size_t)(m + 4) * sys.nl);
}
// BiCGStab(L)'s vectors r_0..r_L, u_0..u_L, r~ (L = 2) for vectors of nl entries, zeroed (kept where they exist)
int ensure_bcgsl_vecs(wai_ctx* c, KrylovVecs& k, size_t nl) {
  if (k.bl) return 0;
  return k.bl.alloc_zeroed(c, BCGSL_VECS * (nl + 16));
}
// a system's matrix: the mesh's pattern with its own block size and values
Bcsr matrix_on(const Pattern& p, int bs, double* val) {
  Bcsr A;
  A.n = p.n; A.ncols = p.ncols; A.nnzb = p.nnzb; A.W = p.W; A.col = p.col; A.rowptr = p.rowptr;
  A.bs = bs; A.val = val;
  return A;
}
static KspOpts ksp_of(const wai_solver_opts& o) {
  KspOpts k;
  k.type = o.ksp_type; k.restart = o.gmres_restart; k.max_its = o.ksp_max_its; k.rtol = o.ksp_rtol; k.atol = o.ksp_atol;
  return k;
}

// events and streams, then the communicator: after the context's device buffers (context.hpp)
Handles::~Handles() {
  for (hipEvent_t e : {ev0, ev1, ev_scal, ev_pack, ev_halo}) if (e) (void)hipEventDestroy(e);
  if (comm_stream) (void)hipStreamDestroy(comm_stream);
  for (hipEvent_t e : {pev0, pev1}) if (e) (void)hipEventDestroy(e);
  if (stream) (void)hipStreamDestroy(stream);
  comm_destroy(comm);
}

}  // namespace wai

// ---- wai_ctx_create's steps, in the order it takes them ----------------------------------------------------------
static int create_handles(wai_ctx* c, int device) {
  c->device = device;
  HIPCHK(c, hipSetDevice(device));
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) c->n_cu = ncu;
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds > 0) c->lds_per_block = (size_t)lds;
  }
  HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIPCHK(c, hipEventCreate(&c->ev0)); HIPCHK(c, hipEventCreate(&c->ev1));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_scal, hipEventDisableTiming));
  HIPCHK(c, hipEventCreate(&c->pev0)); HIPCHK(c, hipEventCreate(&c->pev1));
  return 0;
}

static int create_eos(wai_ctx* c, const wai_eos_desc* ed) {
  c->kind = ed->kind;
  EosTraits et;
  if (eos_traits(c->kind, et)) { c->err = "unsupported eos kind"; return -2; }
  c->np = et.np; c->df = et.df; c->nmob = et.nmob; c->salt = et.salt;
  std::memset(&c->ep, 0, sizeof(c->ep));
  c->ep.temperature = ed->temperature;
  const double ps = ed->pressure_scale > 0 ? ed->pressure_scale : 1.e6;
  const double ts = ed->temperature_scale > 0 ? ed->temperature_scale : 1.e2;
  c->ep.scale[1][0] = ps; c->ep.scale[1][1] = ts;
  c->ep.scale[2][0] = ps; c->ep.scale[2][1] = ts;
  c->ep.scale[4][0] = ps; c->ep.scale[4][1] = 1.0;
  // eos.primary.scale.partial_pressure: absent/<= 0 = adaptive Pg/P (eos_wge.F90:95-104)
  const double gs = ed->partial_pressure_scale > 0 ? ed->partial_pressure_scale : 0.0;
  c->ep.scale[1][2] = gs; c->ep.scale[2][2] = gs; c->ep.scale[4][2] = gs;
  if (c->salt) {
    // eos_wse.F90:155-165, eos_wsge.F90:118-140: regions 5, 6, 8 scale like 1, 2, 4; salt variable
    // unscaled; gas partial pressure (4th) adaptive Pg / P unless a scale is given
    for (int r : {1, 2, 4}) {
      c->ep.scale[r][2] = 1.0;
      c->ep.scale[r][3] = gs;
      for (int k = 0; k < 4; k++) c->ep.scale[r + 4][k] = c->ep.scale[r][k];
    }
  }
  c->ep.rp_type = ed->rp_type; c->ep.cp_type = ed->cp_type;
  if (ed->thermo != WAI_THERMO_IAPWS && ed->thermo != WAI_THERMO_IFC67) { c->err = "unknown thermodynamic formulation"; return -2; }
  c->ep.thermo = ed->thermo;
  c->ep.t1_max = 350.0;   // wai_set_thermo_extrapolate raises it
  if (ed->perm_type < 0 || ed->perm_type > 2) { c->err = "unknown permeability modifier"; return -2; }
  c->ep.perm_type = ed->perm_type;
  for (int i = 0; i < 3; i++) c->ep.perm_par[i] = ed->perm_par[i];
  for (int i = 0; i < 6; i++) { c->ep.rp_par[i] = ed->rp_par[i]; c->ep.cp_par[i] = ed->cp_par[i]; }
  for (int w = 0; w < 3; w++) {   // default tables of the reference: k_r = S on [0, 1]; P_c = 0
    CurveTable& t = c->ep.tab[w];
    t.n = 2; t.interp = 0;
    t.x[0] = 0.0; t.x[1] = 1.0; t.v[0] = 0.0; t.v[1] = w < 2 ? 1.0 : 0.0;
  }
  return 0;
}

// the mesh's sizes and its SoA rock / volume / face geometry
static int create_geometry(wai_ctx* c, const wai_mesh_desc* md) {
  DeviceMesh& m = c->mesh;
  m.n_owned = md->n_owned; m.n_halo = md->n_halo; m.n_bc = md->n_bc;
  m.n_prim = m.n_owned + m.n_halo; m.n_local = m.n_prim + m.n_bc; m.n_faces = md->n_faces;
  const int NL = m.n_local, NF = m.n_faces;
  if (m.n_owned <= 0) { c->err = "no owned cells"; return -2; }
  std::vector<double> rock((size_t)8 * NL), vol(NL), fg((size_t)5 * NF);
  std::vector<int> fdir(NF);
  for (int i = 0; i < NL; i++) {
    for (int k = 0; k < 8; k++) rock[(size_t)k * NL + i] = md->rock[(size_t)i * 8 + k];
    vol[i] = md->cell_geom[(size_t)i * 4 + 3];
  }
  for (int f = 0; f < NF; f++) {
    const double* g = md->face_geom + (size_t)f * 12;
    fg[f] = g[0]; fg[(size_t)NF + f] = g[1]; fg[(size_t)2 * NF + f] = g[2];
    fg[(size_t)3 * NF + f] = g[3]; fg[(size_t)4 * NF + f] = g[7];
    fdir[f] = (int)std::lround(g[11]);
    if (fdir[f] < 1 || fdir[f] > 3) { c->err = "bad permeability direction"; return -2; }
  }
  if (m.rock.upload(c, rock) || m.vol.upload(c, vol) || m.fgeom.upload(c, fg) || m.fdir.upload(c, fdir)) return -1;
  return 0;
}

// cell -> face adjacency and BCSR / block-ELL pattern: built on the host (mesh_pattern.hpp), uploaded here
static int create_pattern(wai_ctx* c, const wai_mesh_desc* md) {
  DeviceMesh& m = c->mesh;
  MeshPattern mp;
  if (int e = build_mesh_pattern(m.n_owned, m.n_prim, m.n_local, m.n_faces, md->face_cells, mp, c->err)) return e;
  m.max_deg = mp.max_deg;
  Pattern& J = c->pat;
  J.n = m.n_owned; J.ncols = m.n_prim; J.W = mp.W; J.nnzb = mp.nnzb;
  J.h_rowptr = std::move(mp.rowptr);
  J.h_colidx = std::move(mp.colidx);
  if (m.adj_tblk.upload(c, mp.adj_tblk)) return -1;
  {
    std::vector<int> fc(md->face_cells, md->face_cells + (size_t)2 * m.n_faces);
    if (m.face_cells.upload(c, fc)) return -1;
  }
  if (m.adj_face.upload(c, mp.adj_face) || m.adj_other.upload(c, mp.adj_other) || m.adj_blk.upload(c, mp.adj_blk) ||
      m.diag_blk.upload(c, mp.diag) || J.rowptr.upload(c, J.h_rowptr) || J.col.upload(c, mp.ell_col))
    return -1;
  return 0;
}

// the flow system: the Jacobian on that pattern, the network's blocks on top, the solver settings of `opts`
static int create_flow_system(wai_ctx* c, const wai_mesh_desc* md) {
  const int N = c->mesh.n_owned, np = c->np;
  const Pattern& J = c->pat;
  LinSys& flow = c->flow;
  if (flow.val.alloc_zeroed(c, ell_size(np, N, J.W))) return -1;
  flow.A = matrix_on(J, np, flow.val);
  flow.net_blocks = true;
  flow.ksp = ksp_of(c->opts);
  flow.kv = &c->kv;
  c->aux.ksp.type = c->coupled.ksp.type = WAI_KSP_GMRES;   // the auxiliary problem's default (timestepper.F90:2021-2022; wai_set_aux_solver)
  {
    std::vector<int> cs(N, -1);
    if (c->mesh.cell_src.upload(c, cs)) return -1;
  }
  // block-Jacobi subdomains + dependency levels of the ILU(0) factors (symbolic phase, once)
  std::vector<int> sub;
  if (md->sub_ptr && md->n_sub > 0) sub.assign(md->sub_ptr, md->sub_ptr + md->n_sub + 1);
  else sub = {0, N};   // one block per rank: the reference's PCBJACOBI / PCASM default
  return build_schedule(c, c->ilu, J.h_rowptr, J.h_colidx, sub, N, J.W, np, true);
}

// state, work and Krylov vectors
static int create_vectors(wai_ctx* c) {
  const DeviceMesh& m = c->mesh;
  const int NL = m.n_local, np = c->np;
  LinSys& flow = c->flow;
  const size_t nl = (size_t)np * m.n_prim, n = (size_t)np * m.n_owned;
  const size_t fsz = (size_t)c->df * NL;
  if (c->flu.alloc_zeroed(c, fsz) || c->flu_last_iter.alloc(c, fsz) || c->flu_last_step.alloc(c, fsz) ||
      c->flu_pert.alloc(c, (size_t)np * c->df * m.n_prim) || c->hstep.alloc(c, nl))
    return -1;
  {
    std::vector<double> ones(NL, 1.0);  // default region 1 (eos_we.F90:91)
    HIPCHK(c, hipMemcpy(c->flu + (size_t)F_REGION * NL, ones.data(), NL * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->flu + (size_t)F_OLD_REGION * NL, ones.data(), NL * sizeof(double), hipMemcpyHostToDevice));
  }
  for (auto p : {&c->w_y, &c->w_yold, &c->w_delta, &c->w_f, &c->w_lhs, &c->w_a, &c->w_b, &c->w_c, &c->w_lhs2, &c->w_hist,
                 &c->w_hist_prev})
    if (p->alloc_zeroed(c, nl + 16)) return -1;
  flow.n = (int)n; flow.nl = (int)nl;
  if (alloc_krylov_vecs(c, c->kv, nl)) return -1;
  if (c->opts.gmres_restart > MAX_RESTART) { c->err = "gmres restart above 40 is not supported"; return -2; }
  c->kv.basis_m = basis_vectors(c->opts.gmres_restart);   // (a basis of this size on first need: here, wai_set_opts, wai_tracer_solve)
  if ((flow.ksp.type == WAI_KSP_GMRES || flow.ksp.type == WAI_KSP_LGMRES) && ensure_basis(c, flow, c->kv.basis_m)) return -1;
  return 0;
}

// the solvers' scalars and reduction slots, the device flags, the staging buffers
static int create_scalars(wai_ctx* c) {
  Krylov& k = c->ks;
  k.nb_max = std::max(1024, c->ilu.nsub);
  if (k.partials.alloc(c, (size_t)NSLOTS * k.nb_max) || k.scal.alloc_zeroed(c, NSCAL) || k.partials2.alloc(c, (size_t)NSLOTS * FIN_MAXF) ||
      k.started.alloc_zeroed(c, 16))
    return -1;
  partials_clear(c, 0, NSLOTS);   // every reduction slot starts empty (fin_block reads arrival off the data)
  // pinned, coherent, device-mapped: the kernels that finish a BiCGStab iteration write the scalars the host
  // tests straight into h_scal[POST_OFF ..] (wait_post)
  if (k.h_scal.alloc(c, NSCAL, hipHostMallocCoherent | hipHostMallocMapped)) return -1;
  std::memset(k.h_scal, 0, NSCAL * sizeof(double));
  {
    void* dp = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dp, k.h_scal, 0));
    k.d_post = reinterpret_cast<double*>(dp) + POST_OFF;
  }
  if (c->d_flags.alloc(c, 4) || c->d_red.alloc(c, 4096) || c->h_flags.alloc(c, 4) || c->h_red.alloc(c, 64)) return -1;
  HIPCHK(c, hipMemcpy(c->d_flags, FLAGS_RESET, sizeof(FLAGS_RESET), hipMemcpyHostToDevice));
  c->stage_len = std::max((size_t)c->flow.nl, (size_t)c->df * c->mesh.n_local) + 16;
  for (auto& p : c->stage)
    if (p.alloc(c, c->stage_len)) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" {

void wai_default_eos(wai_eos_desc* e, int kind) {
  std::memset(e, 0, sizeof(*e));
  e->kind = kind;
  e->temperature = 20.0;
  e->pressure_scale = 1.e6;
  e->temperature_scale = 1.e2;
  e->rp_type = WAI_RP_LINEAR;
  e->rp_par[0] = 0.0; e->rp_par[1] = 1.0; e->rp_par[2] = 0.0; e->rp_par[3] = 1.0;
  e->cp_type = WAI_CP_ZERO;
  e->partial_pressure_scale = 0.0;
  e->thermo = WAI_THERMO_IAPWS;
  e->perm_type = 0;
}

void wai_default_opts(wai_solver_opts* o) {
  o->ksp_type = WAI_KSP_BCGS;
  o->gmres_restart = 30;
  o->ksp_max_its = 10000;
  o->ksp_rtol = 1.e-5;
  o->ksp_atol = 1.e-50;
  o->max_newton_its = 8;
  o->ftol_rel = 1.e-5; o->ftol_abs = 1.0;
  o->utol_rel = 1.e-10; o->utol_abs = 1.0;
  o->fd_eps = 1.e-8; o->fd_umin = 1.e-2;
  o->min_newton_its = 0;
  o->pc_type = WAI_PC_BJACOBI;
  o->asm_overlap = 1;
  o->ilu_levels = 0;
}

int wai_ctx_create(const wai_mesh_desc* md, const wai_eos_desc* ed, const wai_solver_opts* od,
                   int device, wai_ctx** out) {
  if (!md || !ed || !out) return -2;
  wai_ctx* c = new wai_ctx;
  *out = c;
  if (int e = create_handles(c, device)) return e;
  if (od) c->opts = *od; else wai_default_opts(&c->opts);
  if (int e = create_eos(c, ed)) return e;
  if (int e = create_geometry(c, md)) return e;
  if (int e = create_pattern(c, md)) return e;
  if (int e = create_flow_system(c, md)) return e;
  if (int e = create_vectors(c)) return e;
  return create_scalars(c);
}

int wai_ctx_destroy(wai_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  delete c;
  return 0;
}

const char* wai_last_error(wai_ctx* c) { return c ? c->err.c_str() : "null context"; }

// The compact cell order (cell_order.hpp) of a mesh a host is about to describe -- no context, no device.  perm: room for n
// entries, sub_ptr for n + 1 (there are at most ceil(n / max_rows) subdomains, each of at least one cell); err (may be
// NULL): room for err_len characters, the refusal's text, cut to fit and terminated
int wai_cell_order(int n_cells, int n_faces, const int* face_cells, const double* centroids, int centroid_stride, int max_rows,
                   int* perm, int* n_sub, int* sub_ptr, char* err, int err_len) {
  auto refuse = [&](const std::string& text) {
    if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", text.c_str());
    return -2;
  };
  if (err && err_len > 0) err[0] = 0;
  if (!perm || !n_sub || !sub_ptr || (n_cells > 0 && !centroids) || (n_faces > 0 && !face_cells))
    return refuse("cell order: null argument");
  CellOrder o;
  std::string text;
  if (int e = build_cell_order(n_cells, n_faces, face_cells, centroids, centroid_stride, max_rows, o, text)) {
    refuse(text);
    return e;
  }
  *n_sub = o.n_sub;
  std::copy(o.perm.begin(), o.perm.end(), perm);
  std::copy(o.sub_ptr.begin(), o.sub_ptr.end(), sub_ptr);
  return 0;
}

int wai_set_opts(wai_ctx* c, const wai_solver_opts* o) {
  if (!c || !o) return -2;
  if (o->pc_type < WAI_PC_BJACOBI || o->pc_type > WAI_PC_LU) { c->err = "unknown preconditioner type"; return -2; }
  if (o->ilu_levels < 0 || o->ilu_levels > 8) { c->err = "ILU(k): levels 0..8"; return -2; }
  if (o->pc_type != c->opts.pc_type || o->asm_overlap != c->opts.asm_overlap || o->ilu_levels != c->opts.ilu_levels) pc_invalidate(c);
  if (o->gmres_restart > MAX_RESTART) { c->err = "gmres restart above 40 is not supported"; return -2; }
  c->opts = *o;
  c->flow.ksp = ksp_of(c->opts);
  if ((o->ksp_type == WAI_KSP_GMRES || o->ksp_type == WAI_KSP_LGMRES) && ensure_basis(c, c->flow, basis_vectors(o->gmres_restart))) return -1;
  return 0;
}

int wai_num_fluid_dof(wai_ctx* c) { return c ? c->df : -2; }
int wai_block_size(wai_ctx* c) { return c ? c->np : -2; }

int wai_set_sub_pc(wai_ctx* c, int sub) {
  if (!c) return -2;
  if (sub != WAI_SUB_ILU && sub != WAI_SUB_LU) { c->err = "unknown sub-preconditioner (WAI_SUB_ILU or WAI_SUB_LU)"; return -2; }
  if (sub != c->sub_pc) pc_invalidate(c);   // (the cached extended systems are rebuilt by the next set-up: do_pc_setup)
  c->sub_pc = sub;
  return 0;
}

int wai_set_pc_ordering(wai_ctx* c, int ordering) {
  if (!c) return -2;
  if (ordering != WAI_PC_ORDER_NATURAL && ordering != WAI_PC_ORDER_MULTICOLOUR) {
    c->err = "unknown preconditioner ordering (WAI_PC_ORDER_NATURAL or WAI_PC_ORDER_MULTICOLOUR)";
    return -2;
  }
  if (ordering != c->pc_ordering) pc_invalidate(c);   // (what the setting refuses is refused by the next set-up: do_pc_setup)
  c->pc_ordering = ordering;
  return 0;
}
int wai_get_pc_ordering(wai_ctx* c, int* ordering, int* max_colours) {
  if (!c) return -2;
  if (ordering) *ordering = c->pc_ordering;
  if (max_colours) *max_colours = c->colour.built ? c->colour.max_colours : 0;
  return 0;
}

int wai_set_pc_coarse(wai_ctx* c, int mode, int nc, const int* agg) {
  if (!c) return -2;
  if (mode != WAI_PC_COARSE_OFF && mode != WAI_PC_COARSE_ADDITIVE && mode != WAI_PC_COARSE_DEFLATED) {
    c->err = "unknown coarse-level mode (WAI_PC_COARSE_OFF, WAI_PC_COARSE_ADDITIVE or WAI_PC_COARSE_DEFLATED)";
    return -2;
  }
  if (mode == WAI_PC_COARSE_OFF) {
    if (c->coarse.mode != mode) pc_invalidate(c);
    c->coarse.mode = mode;
    return 0;
  }
  // refused by name, from the arguments and settings alone; what was in force stays in force
  if (const char* met = coarse_refusal(c, false)) {
    c->err = std::string("wai_set_pc_coarse: the coarse level serves the flow system under bjacobi or asm on one rank; it met ") + met;
    return -2;
  }
  if (!agg) { c->err = "wai_set_pc_coarse: no aggregates"; return -2; }
  const Pattern& J = c->pat;
  CoarseSpace h;
  std::string text;
  if (int e = build_coarse_space(J.h_rowptr, J.h_colidx, J.n, std::vector<int>(agg, agg + J.n), nc, c->np, h, text)) {
    c->err = "wai_set_pc_coarse: " + text;
    return e;
  }
  pc_invalidate(c);
  c->coarse.mode = WAI_PC_COARSE_OFF;   // (nothing half-made is in force if the upload fails)
  c->coarse.h = std::move(h);
  if (coarse_upload(c)) return -1;
  c->coarse.mode = mode;
  return 0;
}
int wai_get_pc_coarse(wai_ctx* c, int* mode, int* nc) {
  if (!c) return -2;
  if (mode) *mode = c->coarse.mode;
  if (nc) *nc = c->coarse.mode != WAI_PC_COARSE_OFF ? c->coarse.h.nc : 0;
  return 0;
}

int wai_set_pc_tiles(wai_ctx* c, int n_tiles, const int* tile_ptr) {
  if (!c) return -2;
  if (n_tiles < 0) { c->err = "wai_set_pc_tiles: n_tiles < 0"; return -1; }
  const Pattern& J = c->pat;
  std::vector<int> tiles;
  if (n_tiles > 0 && tile_ptr) {
    tiles.assign(tile_ptr, tile_ptr + n_tiles + 1);
    if (check_tiles(tiles, c->ilu.sub, J.n, c->err)) return -1;
  }
  // what depends on the tiles goes: the factor in force, the extended systems (built again by the next set-up: do_pc_setup)
  // and the tile tables of the systems' own schedule, which is made again here
  pc_invalidate(c);
  c->flow.as = AsmSystem(); c->aux.as = AsmSystem(); c->coupled.as = AsmSystem();
  c->pc_tiles.swap(tiles);
  c->ilu.tiles.clear();
  if (c->pc_tiles.empty() || !c->ilu.big) return 0;
  const std::vector<int> sub = c->ilu.sub, id = tile_of_rows(c->pc_tiles, J.n);
  return build_schedule(c, c->ilu, J.h_rowptr, J.h_colidx, sub, J.n, J.W, c->np, true, true, false, false, &id);
}

int wai_set_regions(wai_ctx* c, const int* region) {
  if (!c || !region) return -2;
  const int n = c->mesh.n_prim;
  std::vector<double> r(n);
  for (int i = 0; i < n; i++) r[i] = (double)region[i];
  const size_t NL = c->mesh.n_local;
  HIPCHK(c, hipMemcpy(c->flu + (size_t)F_REGION * NL, r.data(), n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->flu + (size_t)F_OLD_REGION * NL, r.data(), n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int wai_get_regions(wai_ctx* c, int* region) {
  if (!c || !region) return -2;
  const int n = c->mesh.n_prim;
  std::vector<double> r(n);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(r.data(), c->flu + (size_t)F_REGION * c->mesh.n_local, n * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) region[i] = (int)std::lround(r[i]);
  return 0;
}

// Fritsch-Carlson derivatives of a PCHIP table (src/interpolation.F90:810-885, after SLATEC's PCHIM)
static void pchip_derivatives(int n, const double* x, const double* f, double* d) {
  auto sign_test = [](double a, double b) { return (a > 0.0 && b > 0.0) || (a < 0.0 && b < 0.0) ? 1 : ((a == 0.0 || b == 0.0) ? 0 : -1); };
  if (n == 1) { d[0] = 0.0; return; }
  double h1 = x[1] - x[0], del1 = (f[1] - f[0]) / h1;
  if (n == 2) { d[0] = d[1] = del1; return; }
  double h2 = x[2] - x[1], del2 = (f[2] - f[1]) / h2, hsum = h1 + h2;
  double w1 = (h1 + hsum) / hsum, w2 = -h1 / hsum;
  d[0] = w1 * del1 + w2 * del2;
  if (sign_test(d[0], del1) <= 0) d[0] = 0.0;
  else if (sign_test(del1, del2) < 0) { const double dmax = 3.0 * del1; if (std::fabs(d[0]) > std::fabs(dmax)) d[0] = dmax; }
  for (int i = 1; i < n - 1; i++) {
    if (i > 1) { h1 = h2; h2 = x[i + 1] - x[i]; hsum = h1 + h2; del1 = del2; del2 = (f[i + 1] - f[i]) / h2; }
    if (sign_test(del1, del2) > 0) {
      w1 = (hsum + h1) / (3.0 * hsum); w2 = (hsum + h2) / (3.0 * hsum);
      const double dmax = std::max(std::fabs(del1), std::fabs(del2)), dmin = std::min(std::fabs(del1), std::fabs(del2));
      d[i] = dmin / (w1 * (del1 / dmax) + w2 * (del2 / dmax));
    } else d[i] = 0.0;
  }
  w1 = -h2 / hsum; w2 = (h2 + hsum) / hsum;
  d[n - 1] = w1 * del1 + w2 * del2;
  if (sign_test(d[n - 1], del2) <= 0) d[n - 1] = 0.0;
  else if (sign_test(del1, del2) < 0) { const double dmax = 3.0 * del2; if (std::fabs(d[n - 1]) > std::fabs(dmax)) d[n - 1] = dmax; }
}

int wai_set_curve_table(wai_ctx* c, int which, int interpolation, int n, const double* xy) {
  if (!c || !xy) return -2;
  if (which < 0 || which > 2 || n < 1 || n > MAX_CURVE_POINTS || interpolation < 0 || interpolation > 2) {
    c->err = "curve table: which 0..2, 1..12 points, interpolation 0..2";
    return -2;
  }
  CurveTable& t = c->ep.tab[which];
  t.n = n; t.interp = interpolation;
  for (int i = 0; i < n; i++) {
    t.x[i] = xy[2 * i]; t.v[i] = xy[2 * i + 1]; t.d[i] = 0.0;
    if (i > 0 && !(t.x[i] > t.x[i - 1])) { c->err = "curve table coordinates must increase strictly"; return -2; }
  }
  if (interpolation == WAI_INTERP_PCHIP) pchip_derivatives(n, t.x, t.v, t.d);
  return 0;
}

// "thermodynamics.extrapolate" (thermodynamics_setup.F90:57-89): region 1's upper temperature bound 360 instead of 350 deg C
// (IAPWS.F90:449-482, IFC67.F90:228-248), the formulas as they are; a field of the EOS description every launch carries
int wai_set_thermo_extrapolate(wai_ctx* c, int on) {
  if (!c) return -2;
  c->ep.t1_max = on ? 360.0 : 350.0;
  return 0;
}

int wai_get_thermo_extrapolate(wai_ctx* c, int* on) {
  if (!c || !on) return -2;
  *on = c->ep.t1_max > 350.0 ? 1 : 0;
  return 0;
}

int wai_set_bc(wai_ctx* c, const double* primary, const int* region) {
  if (!c) return -2;
  const int nb = c->mesh.n_bc, np = c->np;
  if (nb == 0) return 0;
  if (!primary || !region) return -2;
  const size_t NL = c->mesh.n_local;
  const int first = c->mesh.n_prim;
  std::vector<double> reg(nb), ys((size_t)(first + nb) * np, 0.0);
  for (int b = 0; b < nb; b++) {
    const int rg = region[b];
    const int rmax = c->salt ? 8 : 4;
    if (rg < 1 || rg > rmax || rg == 3 || rg == 7) { c->err = "bad bc region"; return -2; }
    reg[b] = (double)rg;
    for (int k = 0; k < np; k++) {
      const double sc = c->ep.scale[rg][k];
      ys[(size_t)(first + b) * np + k] = (sc == 0.0) ? primary[(size_t)b * np + k] / primary[(size_t)b * np]
                                                     : primary[(size_t)b * np + k] / sc;
    }
  }
  HIPCHK(c, hipMemcpy(c->flu + (size_t)F_REGION * NL + first, reg.data(), nb * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->flu + (size_t)F_OLD_REGION * NL + first, reg.data(), nb * sizeof(double), hipMemcpyHostToDevice));
  DevBuf<double> tmp;
  if (tmp.upload(c, ys)) return -1;
  launch_eos(c, tmp, first, nb, false);
  int fl[4];
  if (fetch_flags(c, fl)) return -1;
  c->bc_set = true;
  return fl[0] ? 1 : 0;
}

// Time-dependent rock properties (rock controls, src/rock_control.F90:49-116, applied by
// flow_simulation_update_rock_properties before every try, src/flow_simulation.F90:2040-2090): one field of the
// 8-double rock record (0..2 permeability, 3 wet / 4 dry conductivity, 5 porosity, 6 density, 7 specific heat) set
// on the listed local cells.
int wai_update_rock(wai_ctx* c, int field, int n, const int* cells, const double* values) {
  if (!c || n < 0 || (n > 0 && (!cells || !values))) return -2;
  if (field < 0 || field > 7) { c->err = "rock field 0..7"; return -2; }
  const int NL = c->mesh.n_local;
  for (int i = 0; i < n; i++) if (cells[i] < 0 || cells[i] >= NL) { c->err = "rock cell out of range"; return -2; }
  if (!n) return 0;
  // a rock type's cells are few thousand at most and change once per try: plane by host round trip
  std::vector<double> plane((size_t)NL);
  HIPCHK(c, hipMemcpyAsync(plane.data(), c->mesh.rock + (size_t)field * NL, sizeof(double) * NL, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; i++) plane[cells[i]] = values[i];
  HIPCHK(c, hipMemcpyAsync(c->mesh.rock + (size_t)field * NL, plane.data(), sizeof(double) * NL, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int wai_set_halo(wai_ctx* c, int n_nbr, const int* nbr_rank, const int* send_ptr, const int* send_idx,
                 const int* recv_ptr) {
  if (!c || n_nbr < 0) return -2;
  c->n_nbr = n_nbr;
  c->nbr_rank.assign(nbr_rank, nbr_rank + n_nbr);
  c->send_ptr.assign(send_ptr, send_ptr + n_nbr + 1);
  c->recv_ptr.assign(recv_ptr, recv_ptr + n_nbr + 1);
  c->send_total = n_nbr ? send_ptr[n_nbr] : 0;
  if (n_nbr && recv_ptr[n_nbr] != c->mesh.n_halo) { c->err = "recv_ptr does not cover the halo cells"; return -2; }
  std::vector<int> idx(send_idx, send_idx + c->send_total);
  for (int v : idx) if (v < 0 || v >= c->mesh.n_owned) { c->err = "send_idx not an owned cell"; return -2; }
  c->max_dof_buf = std::max(c->np, 1);
  if (c->d_send_idx.upload(c, idx) || c->d_sendbuf.alloc(c, (size_t)c->send_total * c->max_dof_buf) ||
      c->d_recvbuf.alloc(c, (size_t)c->mesh.n_halo * c->max_dof_buf))
    return -1;
  return 0;
}

int wai_comm_unique_id(char id[128]) {
  std::string err;
  return comm_unique_id(id, err);
}

int wai_comm_init(wai_ctx* c, int rank, int nranks, const char id[128]) {
  if (!c) return -2;
  HIPCHK(c, hipSetDevice(c->device));
  comm_destroy(c->comm);
  c->comm = comm_create(rank, nranks, id, c->err);
  if (!c->comm) return -1;
  // Halo exchange behind the interior bricks: on by default (WAI_HALO_OVERLAP=0: in-order exchange).
  // MEASURED on one GPU at 108^3 (one rank's share of the 8-GPU run): fused kernel 96.9 us in one
  // launch, 54.3 us (interior bricks) + 51.5 us (face bricks) in two -- splitting costs 8.9 us per
  // application, and the interior launch is long enough to cover three 187-KB xGMI messages and RCCL's
  // send/recv launch latency, which the in-order exchange exposes in full twice per BiCGStab iteration.
  // (The tests' loopback transport time-slices all ranks on one GPU and switches it off.)
  const char* ov = getenv("WAI_HALO_OVERLAP");
  if (nranks > 1 && !c->comm_stream && !(ov && ov[0] == '0')) {
    // highest priority: the interior bricks fill every CU at full occupancy, and RCCL's send / receive kernels, the
    // pack and the unpack must not queue behind them -- they are what the face bricks wait for
    int prio_lo = 0, prio_hi = 0;
    HIPCHK(c, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    HIPCHK(c, hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, prio_hi));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_pack, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_halo, hipEventDisableTiming));
  }
  return 0;
}

}  // extern "C"
