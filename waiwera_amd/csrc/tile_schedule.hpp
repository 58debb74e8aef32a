// The symbolic phase of the tile-scheduled substitution sweeps for subdomains of more than a workgroup's rows (a `big`
// schedule, ilu_schedule.hpp): the subdomain is cut into TILES of at most 1024 consecutive rows -- wai_set_pc_tiles; the
// mesh's bricks are such tiles -- and the tiles form a dependency graph of their own.  Rows ascend and tiles are
// contiguous, so a tile's lower couplings reach only lower-numbered tiles: one launch per TILE level gives every tile of
// that level one workgroup, which walks the tile's own row levels with barriers (k_tile_solve, kernels_factor.hip), and
// couplings that leave the tile read what earlier launches finished.  Pure host code -- no device header, no context -- so
// that a plain C++ program can call it (tests/tile_schedule_host); build_schedule (pc_setup.hip) uploads what
// build_tile_schedule makes.  Not part of the ABI.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace wai {

constexpr int MAX_TILE_ROWS = 1024;   // one thread per row of a tile, one workgroup per tile

// What a tile schedule says besides its tables: TileTables (context.hpp) is these facts plus the tables on the device.
struct TileFacts {
  int n_tiles = 0;                 // 0: the schedule has no tiles
  int ntl_f = 0, ntl_b = 0;        // tile levels of the forward / backward sweep: launches per sweep
  int max_tile_rows = 0;           // rows of the largest tile: threads of the workgroup, whole waves
  int max_in_levels = 0;           // most in-tile levels of any tile, either way
  // do the tile sweeps take fewer launches than the level sweeps: ntl_f + ntl_b < nlev_f + nlev_b?  A tiling that is a
  // chain (every tile waits for the one before it) would cost more launches than rows have levels and keeps the level path
  bool serve = false;
  std::vector<int> tl_f_ptr, tl_b_ptr;   // tile ranges of each tile level in ord_f / ord_b
};

// The facts and every table as the device gets it.
struct HostTiles : TileFacts {
  std::vector<int> tile_ptr;       // [n_tiles + 1] row ranges
  std::vector<int> tile_lev;       // [n_tiles] forward level | backward level << 16
  std::vector<int> tile_nin;       // [n_tiles] in-tile levels: forward | backward << 16
  std::vector<int> ord_f, ord_b;   // tiles sorted by forward level, by backward level
  std::vector<int> row_lev;        // [N] in-tile level of the row: forward | backward << 16
};

// wai_set_pc_tiles' refusals: tile_ptr[n_tiles + 1] must ascend from 0 to N, no tile empty or of more than 1024 rows, every
// subdomain boundary (sub[0] = 0 <= .. <= sub[nsub] = N) a tile boundary.  Returns 0, or -1 with `err` naming the tile.
inline int check_tiles(const std::vector<int>& tile_ptr, const std::vector<int>& sub, int N, std::string& err) {
  const int nt = (int)tile_ptr.size() - 1;
  auto refuse = [&](const std::string& what) { err = "wai_set_pc_tiles: " + what; return -1; };
  if (nt < 1) return refuse("tile_ptr must ascend from 0 to n_owned (no tile)");
  if (tile_ptr[0] != 0) return refuse("tile_ptr must ascend from 0 to n_owned (tile 0 starts at row " + std::to_string(tile_ptr[0]) + ")");
  for (int t = 0; t < nt; t++) {
    const int lo = tile_ptr[t], hi = tile_ptr[t + 1];
    if (hi < lo) return refuse("tile_ptr must ascend from 0 to n_owned (tile " + std::to_string(t) + " ends before it starts)");
    if (hi == lo) return refuse("tile " + std::to_string(t) + " is empty");
    if (hi - lo > MAX_TILE_ROWS)
      return refuse("tile " + std::to_string(t) + " has " + std::to_string(hi - lo) + " rows, more than " + std::to_string(MAX_TILE_ROWS));
    if (hi > N) return refuse("tile_ptr must ascend from 0 to n_owned (tile " + std::to_string(t) + " ends at row " + std::to_string(hi) + ")");
  }
  if (tile_ptr[nt] != N)
    return refuse("tile_ptr must ascend from 0 to n_owned (tile " + std::to_string(nt - 1) + " ends at row " + std::to_string(tile_ptr[nt]) + ")");
  for (int t = 0, sd = 0; t < nt; t++) {
    while (sd + 1 < (int)sub.size() && sub[sd + 1] <= tile_ptr[t]) sd++;   // the subdomain of the tile's first row
    if (sd + 1 < (int)sub.size() && tile_ptr[t + 1] > sub[sd + 1])
      return refuse("tile " + std::to_string(t) + " straddles a subdomain boundary (row " + std::to_string(sub[sd + 1]) + ")");
  }
  return 0;
}

// counting sort of the tiles by level: the tiles of level l are ord[ptr[l] .. ptr[l + 1]), ascending
inline void tiles_by_level(const std::vector<int>& lev, int nlev, std::vector<int>& ptr, std::vector<int>& ord) {
  ptr.assign(nlev + 1, 0);
  ord.resize(lev.size());
  for (int l : lev) ptr[l + 1]++;
  for (int l = 0; l < nlev; l++) ptr[l + 1] += ptr[l];
  std::vector<int> pos(ptr.begin(), ptr.end() - 1);
  for (int t = 0; t < (int)lev.size(); t++) ord[pos[lev[t]]++] = t;
}

// The tile schedule of the N x N factor pattern (rowptr, colidx, ascending columns) under the subdomains `sub`.
// info: per row the big schedule's descriptor lfirst | dslot << 8 | ulast << 16 -- the L part in slots [lfirst, dslot), the U
//   part in (dslot, ulast), in-subdomain columns only.
// row_tile: a tile id per row.  A tile is a run of consecutive rows of one subdomain with one id: a system's own schedule
//   passes the row's tile; an extended system (PCASM, ILU(k)) the tile of the original row each of its rows stands for --
//   its blocks hold their rows in ascending original order, so an original tile's rows are contiguous inside a block, and
//   the same id in two blocks gives two tiles.
// nlev_f, nlev_b: the row levels of the level path, for `serve`.
// Returns 0, or -2 with `err` set (a run of more than 1024 rows; more than 65535 levels); `out` is built from nothing.
inline int build_tile_schedule(const std::vector<int>& rowptr, const std::vector<int>& colidx, const std::vector<int>& sub,
                               const std::vector<int>& info, const std::vector<int>& row_tile, int N, int nlev_f, int nlev_b,
                               HostTiles& out, std::string& err) {
  out = HostTiles();
  if ((int)row_tile.size() != N || (int)info.size() != N || N < 1) { err = "tile schedule: one tile id and one descriptor per row"; return -2; }
  std::vector<int> tile(N);   // the tile of every row
  for (int sd = 0; sd + 1 < (int)sub.size(); sd++)
    for (int i = sub[sd]; i < sub[sd + 1]; i++) {
      if (i == sub[sd] || row_tile[i] != row_tile[i - 1]) out.tile_ptr.push_back(i);
      tile[i] = (int)out.tile_ptr.size() - 1;
    }
  out.tile_ptr.push_back(N);
  const int nt = (int)out.tile_ptr.size() - 1;
  for (int t = 0; t < nt; t++) {
    const int rows = out.tile_ptr[t + 1] - out.tile_ptr[t];
    if (rows > MAX_TILE_ROWS) { err = "tile schedule: a tile of " + std::to_string(rows) + " rows, more than " + std::to_string(MAX_TILE_ROWS); return -2; }
    out.max_tile_rows = std::max(out.max_tile_rows, rows);
  }
  // levels: a tile's is 0 without a predecessor tile, else 1 + the largest among the tiles that hold a coupled row; a
  // row's in-tile level the same recurrence over the couplings that stay in its tile
  std::vector<int> tlf(nt, 0), tlb(nt, 0), inf(N, 0), inb(N, 0), ninf(nt, 0), ninb(nt, 0);
  for (int i = 0; i < N; i++) {
    const int* row = colidx.data() + rowptr[i];
    const int lfirst = info[i] & 255, dslot = (info[i] >> 8) & 255, t = tile[i];
    for (int q = lfirst; q < dslot; q++) {
      const int k = row[q];
      if (tile[k] == t) inf[i] = std::max(inf[i], inf[k] + 1);
      else tlf[t] = std::max(tlf[t], tlf[tile[k]] + 1);
    }
    ninf[t] = std::max(ninf[t], inf[i] + 1);
  }
  for (int i = N - 1; i >= 0; i--) {
    const int* row = colidx.data() + rowptr[i];
    const int dslot = (info[i] >> 8) & 255, ulast = info[i] >> 16, t = tile[i];
    for (int q = dslot + 1; q < ulast; q++) {
      const int k = row[q];
      if (tile[k] == t) inb[i] = std::max(inb[i], inb[k] + 1);
      else tlb[t] = std::max(tlb[t], tlb[tile[k]] + 1);
    }
    ninb[t] = std::max(ninb[t], inb[i] + 1);
  }
  // (a tile's level is read only by later tiles, whose rows all come after its own: it is final by then; tlb likewise, descending)
  out.n_tiles = nt;
  out.ntl_f = *std::max_element(tlf.begin(), tlf.end()) + 1;
  out.ntl_b = *std::max_element(tlb.begin(), tlb.end()) + 1;
  out.max_in_levels = std::max(*std::max_element(ninf.begin(), ninf.end()), *std::max_element(ninb.begin(), ninb.end()));
  if (out.max_in_levels > 0xffff || out.ntl_f > 0xffff || out.ntl_b > 0xffff) { err = "tile schedule: more than 65535 levels"; return -2; }
  out.serve = out.ntl_f + out.ntl_b < nlev_f + nlev_b;
  out.tile_lev.resize(nt); out.tile_nin.resize(nt); out.row_lev.resize(N);
  for (int t = 0; t < nt; t++) { out.tile_lev[t] = tlf[t] | (tlb[t] << 16); out.tile_nin[t] = ninf[t] | (ninb[t] << 16); }
  for (int i = 0; i < N; i++) out.row_lev[i] = inf[i] | (inb[i] << 16);
  tiles_by_level(tlf, out.ntl_f, out.tl_f_ptr, out.ord_f);
  tiles_by_level(tlb, out.ntl_b, out.tl_b_ptr, out.ord_b);
  return 0;
}

// the tile id of every row from wai_set_pc_tiles' row ranges
inline std::vector<int> tile_of_rows(const std::vector<int>& tile_ptr, int N) {
  std::vector<int> id(N, 0);
  for (int t = 0; t + 1 < (int)tile_ptr.size(); t++)
    for (int i = tile_ptr[t]; i < tile_ptr[t + 1] && i < N; i++) id[i] = t;
  return id;
}

}  // namespace wai
