// tl_grid_plan.hpp -- how a build of the search grids sizes its cells, lays out its tables and scans them, decided by one
// function (DESIGN.md section 4 has the table), and which scan an array of counts takes anywhere in the library.
// Host only, plain C++17, no HIP: tests/host/grid_plan_main.cpp includes it alone.  build_grids_over (tl_api_frames.hip) fills a
// GridPlanIn from the boxes, keeps plan_grids' answer and switches on it; the scans' launchers (tl_scan.hip) and everybody who
// reserves a scan's scratch ask scan_path.  The size limits are the constants below; the kernel files take them from here.
#pragma once

#include <stddef.h>

#include <algorithm>
#include <cmath>

namespace tl {

// ---- the size limits -----------------------------------------------------------------------------------------------
constexpr int kScanTile = 2048;          // elements a block of the tile scan takes (k_scan_tile: 256 threads x 8)
constexpr int kSmallTile = 16384;        // elements ONE block of 1024 threads scans per round (k_scan_small): up to here, one launch
constexpr int kTile1p = 16384;           // elements a block of the single-pass scan holds in registers (k_scan_1p)
constexpr int kScanLdsTiles = 1024;      // most tiles whose offsets a fused consumer forms in LDS (tile_offsets_to_lds)
constexpr int kScan1pSpareCus = 16;      // the single-pass scan leaves 1 / 16 of the CUs to whatever else runs on the device
constexpr double kGridCellsPerPoint = 32.0;   // cells per target point a sparse kind's table may have before its cell grows ...
constexpr double kGridSparseFloor = 16384.0;  // ... never below 16 Ki cells (measured at 16 / 32 / 64: profiles/grid_tables_time.json)
constexpr double kGridMaxCells = 4.0e6;       // cells of any kind's table
constexpr double kGridCellGrowth = 1.25;      // factor a cell grows by until its table fits
constexpr double kGridRadiusSlack = 1.0 + 1e-6;   // cell >= radius * this: every target within `radius` of a query lies in its 27 cells
constexpr int kGridKinds = 4;

// ---- which scan an array of `entries` counts takes ---------------------------------------------------------------------
enum class ScanPath {
  ONE_BLOCK,     // at most kSmallTile entries: k_scan_small
  TILES,         // at most kScanLdsTiles tiles: k_scan_tile, then the consumer (or k_scan_add_direct) adds the tiles' offsets
  SINGLE_PASS,   // more tiles, and every 16 Ki block resident at once on this device: one look-back launch (k_scan_1p)
  MULTI_LAUNCH   // more tiles otherwise: tile scan, scan of the totals, add
};
struct ScanChoice {
  ScanPath path;
  int tiles;   // TILES: the tile count; 0 otherwise
};
inline size_t scan_tiles(size_t entries) { return (entries + kScanTile - 1) / kScanTile; }
inline size_t scan_1p_tiles(size_t entries) { return (entries + kTile1p - 1) / kTile1p; }
inline ScanChoice scan_path(size_t entries, int device_cus, bool single_pass_allowed) {
  if (entries <= (size_t)kSmallTile) return {ScanPath::ONE_BLOCK, 0};
  const size_t tiles = scan_tiles(entries);
  if (tiles <= (size_t)kScanLdsTiles) return {ScanPath::TILES, (int)tiles};
  // (at most one 16 Ki block per CU of THIS device, less the spare ones: all resident at once, so a block of the look-back only
  //  waits for blocks that run; a partition or a CU-masked device reports fewer CUs and takes the multi-launch scan)
  const bool resident = (long long)scan_1p_tiles(entries) <= (long long)(device_cus - device_cus / kScan1pSpareCus);
  return {single_pass_allowed && resident ? ScanPath::SINGLE_PASS : ScanPath::MULTI_LAUNCH, 0};
}
// u64 of scratch the multi-launch scan of `entries` takes: totals and their scan, level by level
inline size_t scan_scratch_elems(size_t entries) {
  size_t total = 0;
  while (entries > 1) {
    const size_t tiles = scan_tiles(entries);
    total += 2 * tiles;
    if (tiles == 1) break;
    entries = tiles;
  }
  return total + 16;
}
// control words of the single-pass scan of `entries` (zero when allocated, never cleared)
inline size_t scan_ctl_elems(size_t entries) { return scan_1p_tiles(entries) + 8; }
// a table whose size follows the bounding boxes grows with room to spare: a re-allocation inside a frame costs ~0.7 ms
inline size_t grown(size_t n, bool has_to_grow) { return has_to_grow ? 2 * n + 64 : n; }

// ---- the plan of one build -------------------------------------------------------------------------------------------
struct GridPlanIn {
  double lo[kGridKinds][3], hi[kGridKinds][3];   // the clouds' boxes over their finite points (lo > hi: not one finite point)
  long long n[kGridKinds];                       // points
  double radius[kGridKinds];                     // <= 0: the kind is not built
  bool sparse_ok;             // the context's caps admit no direct set: a kind's table is also bounded by its point count
  int device_cus;
  bool single_pass_allowed;   // the context has not fallen back to the multi-launch scans
};
inline bool grid_kind_built(double radius, long long n) { return radius > 0.0 && n > 0; }
enum class GridScan { NONE = 0, SMALL = 1, TILES = 2, SINGLE_PASS = 3, GENERIC = 4 };   // == TLOAM_GRID_SCAN_*
struct GridPlan {
  struct Kind {
    int n;         // points gridded: 0 for a kind with radius <= 0, no points, or an empty or inverted box
    int tgt_off;   // the kind's place in the concatenated point arrays (a kind dropped for its box keeps its place)
    double cell, inv_cell, org[3];
    int dim[3];
    long long ncell;
    long long cell_base;    // the kind's first entry in the histogram (and in the scan)
    long long start_base;   // ... and in cell_start: ncell + 1 entries, the last one the terminator
  } k[kGridKinds];
  long long tgt_total, cell_total;
  long long n_tab;   // entries of the padded table
  GridScan scan;
  int tiles;         // TILES: scan tiles of the padded table
  int elem_bytes;    // of a histogram / scan entry: 4 (TILES), 8, or 0 (NONE)
};
// Two layouts.  PADDED (the TILES path, 32-bit tables): kind k's ncell + 1 entries start on a multiple of 4 in the histogram, the
// scan and cell_start alike -- 16-byte accesses, and the terminator falls out of the scan.  PACKED (every other path, 64-bit
// histogram): cell_base[k] = the cells in front of kind k, and cell_start carries one terminator per kind, so kind k's entries
// sit k places further on.  The single-pass condition is judged on the packed size (cell_total + 1), the tile condition on the
// padded one (n_tab): a table whose packed size fits kScanLdsTiles tiles and whose padded size does not is GENERIC.
inline GridPlan plan_grids(const GridPlanIn& in) {
  GridPlan p{};
  for (int k = 0; k < kGridKinds; ++k) {
    GridPlan::Kind& g = p.k[k];
    g.n = grid_kind_built(in.radius[k], in.n[k]) ? (int)in.n[k] : 0;
    g.tgt_off = (int)p.tgt_total;
    p.tgt_total += g.n;
  }
  for (int k = 0; k < kGridKinds; ++k) {
    GridPlan::Kind& g = p.k[k];
    const double* lo = in.lo[k];
    const double* hi = in.hi[k];
    // (sizing a cell table from the box of a cloud without a finite point was a GPU memory fault once: no grid, like an empty cloud)
    if (g.n > 0 && !(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) g.n = 0;
    if (g.n == 0) { g.dim[0] = g.dim[1] = g.dim[2] = 1; g.inv_cell = 1.0; continue; }
    // Any cell of at least the radius serves (the walk covers the ball, the search is exact k-NN): the bounds trade table bytes
    // against candidates per query, never results -- 1500 sphere targets over a street's volume were 42 % of a frame's table bytes.
    double cell = in.radius[k] * kGridRadiusSlack;
    const double sparse_cap = in.sparse_ok ? std::max(kGridSparseFloor, kGridCellsPerPoint * (double)g.n) : kGridMaxCells;
    double dims[3];
    for (;;) {
      double cells = 1.0;
      for (int a = 0; a < 3; ++a) {
        dims[a] = std::floor((hi[a] - lo[a]) / cell) + 1.0;
        cells *= dims[a];
      }
      if (cells <= kGridMaxCells && cells <= sparse_cap) break;
      cell *= kGridCellGrowth;
    }
    g.cell = cell;
    g.inv_cell = 1.0 / cell;
    g.ncell = 1;
    for (int a = 0; a < 3; ++a) {
      g.org[a] = lo[a];
      g.dim[a] = (int)dims[a];
      g.ncell *= g.dim[a];
    }
    p.cell_total += g.ncell;
  }
  for (int k = 0; k < kGridKinds; ++k) p.n_tab += (p.k[k].ncell + 1 + 3) & ~3ll;
  const ScanChoice packed = scan_path((size_t)std::max(p.cell_total, 1ll) + 1, in.device_cus, in.single_pass_allowed);
  const ScanChoice padded = scan_path((size_t)p.n_tab, in.device_cus, false);
  if (p.cell_total == 0) p.scan = GridScan::NONE;
  else if (packed.path == ScanPath::SINGLE_PASS) p.scan = GridScan::SINGLE_PASS;
  else if (padded.path == ScanPath::TILES) p.scan = GridScan::TILES;
  else p.scan = packed.path == ScanPath::ONE_BLOCK ? GridScan::SMALL : GridScan::GENERIC;
  p.tiles = p.scan == GridScan::TILES ? padded.tiles : 0;
  p.elem_bytes = p.scan == GridScan::NONE ? 0 : p.scan == GridScan::TILES ? 4 : 8;
  long long at = 0;
  for (int k = 0; k < kGridKinds; ++k) {
    GridPlan::Kind& g = p.k[k];
    g.cell_base = at;
    g.start_base = at + (p.tiles > 0 ? 0 : k);   // THE "+ k" of the packed layout
    at += p.tiles > 0 ? ((g.ncell + 1 + 3) & ~3ll) : g.ncell;
  }
  return p;
}

// ---- what the build's buffers are to hold ---------------------------------------------------------------------------
struct GridCaps { size_t cell_start, cell_cnt, cell_cnt32; };   // elements held now, of the buffers the growth conditions look at
struct GridWant {
  size_t n;      // elements the buffer is to hold; 0: this build does not use it
  bool zeroed;   // a (re)allocation is cleared: the histograms and the control words read zero between builds
};
struct GridReservation {   // (in the order the buffers are reserved)
  GridWant gp, cell_of_pt, rank_of_pt, cell_start, cell_cnt32, cell_scan32, totals32, cell_cnt, scan1p, cell_scan, scan_tmp;
};
inline GridReservation grid_reservation(const GridPlan& p, const GridCaps& cap) {
  GridReservation r{};
  const size_t tgt = (size_t)p.tgt_total;
  r.gp = r.cell_of_pt = {std::max<size_t>(tgt, 1), false};
  r.rank_of_pt = {tgt + 1, false};
  if (p.scan == GridScan::TILES) {
    const size_t nt = (size_t)p.n_tab;
    const size_t nt_res = grown(nt, nt > cap.cell_cnt32 || nt > cap.cell_start);
    r.cell_start = {nt_res, false};
    r.cell_cnt32 = {nt_res, true};
    r.cell_scan32 = {nt_res, false};
    r.totals32 = {(size_t)kScanLdsTiles, false};
    return r;
  }
  const size_t nc = (size_t)std::max(p.cell_total, 1ll);   // (a build without a cell still holds its terminators)
  const size_t nc_res = grown(nc, nc + 1 > cap.cell_cnt || nc + kGridKinds + 1 > cap.cell_start);
  r.cell_start = {nc_res + kGridKinds + 1, false};
  r.cell_cnt = {nc_res + 1, true};
  if (p.scan == GridScan::SINGLE_PASS) {
    r.scan1p = {scan_ctl_elems(nc_res + 1), true};
  } else {
    r.cell_scan = {nc_res + 1, false};
    r.scan_tmp = {scan_scratch_elems(nc_res + 1), false};
  }
  return r;
}

}  // namespace tl
