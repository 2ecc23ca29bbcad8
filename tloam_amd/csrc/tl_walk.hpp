// tl_walk.hpp -- knn_rows: one query against the HBM grid of its kind, by LPQ cooperating lanes (1, 4 or 16): the walk of
// K1 (tl_nn.hip: the builders of the registration path, K = 1 / 5) and, since round 4, of the PCA pass of the feature extraction
// (tl_feature.hip, K = 20, LPQ = 1).  Included where TL_K1_STAMP is defined (a development aid of tl_nn.hip; empty elsewhere).
//   LPQ = 1: the lane resolves the nine (z,y) rows of the 27-cell neighbourhood (one 16-byte cell-table
//            request per row, all in flight) and walks them as one candidate stream, four records per trip.
//   LPQ = 4 / 16: smaller frames are latency-bound (a ~35-candidate dependent chain per query), so 4 (16)
//            adjacent lanes resolve the nine rows -- three (at most one) each -- and merge their packed-key
//            lists with two (four) xor-shuffle rounds; lane 0 of the group finishes the fit.
//            LPQ = 4 walks row-owner: every lane its own three rows, two records of each per trip.
//            LPQ = 16 walks the query's rows as ONE run of 16-byte pieces (two per record) dealt to the sixteen
//            lanes in order, so that the lanes of a load instruction cover contiguous bytes: 32 records per trip,
//            the lane pair joins a record's halves, the even lane inserts it.
#pragma once

#include "tl_common.hpp"
#include "tl_knn.hpp"

#ifndef TL_K1_STAMP
#define TL_K1_STAMP(i)
#endif

namespace tl {

// A DPP move inside the sixteen-lane row (one query's lanes at LPQ = 16): CTRL 0x111 .. 0x11F = row_shr:1 .. 15,
// 0x150 .. 0x15F = row_newbcast:0 .. 15 (the value of that lane of the row), 0xB1 = quad_perm:[1,0,3,2] (the lane pair
// swapped); a lane without a source reads 0.
template <int CTRL>
__device__ __forceinline__ int row_dpp(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}

template <int K, int LPQ>
__device__ __forceinline__ void knn_rows(const GridView& g, const PtsGlobal& pts, Vec3 pw, int sub, TopK<K>& tk,
                                         int2* __restrict__ lds_rows, double radius, NbrXyz<K>* xyz = nullptr) {
  TL_K1_STAMP(1)
  const int cx = cell_coord(pw.x, g.org[0], g.inv_cell, g.dim[0]);
  const int cy = cell_coord(pw.y, g.org[1], g.inv_cell, g.dim[1]);
  const int cz = cell_coord(pw.z, g.org[2], g.inv_cell, g.dim[2]);
  int x0 = cx - 1;
  if (x0 < 0) x0 = 0;
  constexpr int NR = (9 + LPQ - 1) / LPQ;  // rows per lane
  int rs[NR], re[NR];
  // CLIPPED walk: only the cells the search ball can reach.  A neighbour is kept only below the radius (radius_cut), so
  // a cell whose nearest point is farther than radius * (1 + 1e-6) from the query holds nothing that can be kept: per
  // axis the distance to the lower / upper neighbour slab follows from the query's position inside its own cell, a row
  // (dy, dz) is walked only if dy^2 + dz^2 <= reach^2 and its outer cells only if the x term still fits.  With
  // cell = radius, on average 20.6 of the 27 cells survive (the volume of cube (+) ball): a quarter of the candidate
  // records is never fetched.  The margin (2e-6 relative on the squares) dwarfs the rounding of these few products.
  const double cl = g.cell, reach = radius * (1.0 + 1e-6), c2 = reach * reach;
  const double fx = (pw.x - g.org[0]) * g.inv_cell - (double)cx, fy = (pw.y - g.org[1]) * g.inv_cell - (double)cy,
               fz = (pw.z - g.org[2]) * g.inv_cell - (double)cz;
  const double dxl = fx * cl, dxr = (1.0 - fx) * cl, dyl = fy * cl, dyr = (1.0 - fy) * cl, dzl = fz * cl, dzr = (1.0 - fz) * cl;
  const double sxl = dxl * dxl, sxr = dxr * dxr, syl = dyl * dyl, syr = dyr * dyr, szl = dzl * dzl, szr = dzr * dzr;
  // The row's table entries (start of its first cell, end of its last) are at most three ints apart: ONE 16-byte
  // request per row instead of two 4-byte ones.  (Reads up to 12 bytes past the last entry of the table: inside the
  // allocation slack of DBuf.)
  typedef int int4u __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int r = sub + i * LPQ;
    const int rz = r / 3, ry = r % 3;
    const int z = cz - 1 + rz, y = cy - 1 + ry;
    const double s2 = (rz == 0 ? szl : (rz == 2 ? szr : 0.0)) + (ry == 0 ? syl : (ry == 2 ? syr : 0.0));
    int xa = cx - ((s2 + sxl <= c2) ? 1 : 0), xb = cx + ((s2 + sxr <= c2) ? 1 : 0);
    if (xa < 0) xa = 0;
    if (xb >= g.dim[0]) xb = g.dim[0] - 1;
    const bool in = (r < 9) && (s2 <= c2) && (xa <= xb) && z >= 0 && z < g.dim[2] && y >= 0 && y < g.dim[1];
    const size_t base = in ? ((size_t)z * g.dim[1] + y) * g.dim[0] + x0 : 0;
    const int4u t = *reinterpret_cast<const int4u*>(g.cell_start + base);
    const int ia = xa - x0, ib = xb + 1 - x0;  // 0..1, 1..3
    rs[i] = in ? (ia == 0 ? t.x : t.y) : 0;
    re[i] = in ? (ib == 3 ? t.w : (ib == 2 ? t.z : t.y)) : 0;
  }
  topk_clear<K>(tk);
  TL_K1_STAMP(2)
  if (LPQ == 1) {
    // FLATTENED walk: the lane's non-empty rows are queued in LDS ([row][lane], conflict-free) and consumed
    // as ONE candidate stream, two candidates per trip.  The wave then runs max_lanes(total candidates)/2
    // trips instead of sum_rows max_lanes(row length)/2 -- half the trips on the 1 M frame, where the lanes
    // of a wave (one 4x4x4-cell tile) see very different row lengths.
    const int lane = threadIdx.x & 63;
    int nr = 0, total = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int len = re[i] - rs[i];
      if (len > 0) {
        lds_rows[nr * 64 + lane] = int2{rs[i], re[i]};
        ++nr;
        total += len;
      }
    }
    int j = 0, e = 0, r = 0;
    int2 nx = (nr > 0) ? lds_rows[lane] : int2{0, 0};  // next row, pre-loaded
    // (ballot, not a shuffle reduction: the kinds of a wave's lanes may differ, and only a ballot is
    //  well-defined under the divergent kind branch)
    const unsigned keep_mask = ~((1u << key_bits_for(g.n)) - 1u);
    KeyList<K + 1> L;
    keys_clear<K + 1>(L);
    // next position of this lane's candidate stream (index 0 = a harmless in-range dummy when exhausted)
    auto next = [&](int& jx, bool& vx) {
      if (j >= e && r < nr) { j = nx.x; e = nx.y; ++r; nx = lds_rows[(r < nr ? r : 0) * 64 + lane]; }
      vx = j < e;
      jx = vx ? j : 0;
      j += vx ? 1 : 0;
    };
    // kCpt candidates per trip, and the records of the NEXT trip requested before this trip's insertions: with
    // the two-instruction key insertion the walk is bound by the record round trips (PMC: 53 % of the wave
    // cycles waiting on memory at two records in flight), so the trip carries as many independent loads as the
    // register budget allows.
#ifndef TLOAM_K1_CPT
#define TLOAM_K1_CPT 4
#endif
    constexpr int kCpt = TLOAM_K1_CPT;
    int jc[kCpt];
    bool vc[kCpt];
    double4 rc[kCpt];
#pragma unroll
    for (int u = 0; u < kCpt; ++u) next(jc[u], vc[u]);
#pragma unroll
    for (int u = 0; u < kCpt; ++u) rc[u] = pts.p[jc[u]];
#ifdef TLOAM_K1_DBG_NOWALK  // timing experiment only: row resolution and the first trip, no candidate loop
    total = 0;
#endif
#ifdef TLOAM_K1_DBG_MAXTRIPS  // timing experiment only: the walk cut off after a fixed number of trips
    int trip_no = 0;
    for (int left = total; __any(left > 0) && trip_no < TLOAM_K1_DBG_MAXTRIPS; left -= kCpt, ++trip_no) {
#else
    for (int left = total; __any(left > 0); left -= kCpt) {
#endif
      int jn[kCpt];
      bool vn[kCpt];
      double4 rn[kCpt];
#pragma unroll
      for (int u = 0; u < kCpt; ++u) next(jn[u], vn[u]);
#pragma unroll
      for (int u = 0; u < kCpt; ++u) rn[u] = pts.p[jn[u]];
#pragma unroll
      for (int u = 0; u < kCpt; ++u) {
        const double du = sqdist(pw.x, pw.y, pw.z, rc[u].x, rc[u].y, rc[u].z);
        key_insert<K + 1>(L, key_pack(du, jc[u], keep_mask, vc[u]));
      }
#pragma unroll
      for (int u = 0; u < kCpt; ++u) { jc[u] = jn[u]; vc[u] = vn[u]; rc[u] = rn[u]; }
    }
    if (!keys_ambiguous<K + 1>(L, keep_mask)) {
      keys_unpack<K, K + 1>(L, pts, pw.x, pw.y, pw.z, keep_mask, tk, xyz);
    } else {  // two kept distances agree in every mantissa bit the key keeps: redo with the exact (d, original index) order
      topk_clear<K>(tk);
      for (int q = 0; q < nr; ++q) {
        const int2 v = lds_rows[q * 64 + lane];
        scan_range<K>(pts, v.x, v.y, pw.x, pw.y, pw.z, tk);
      }
      if (xyz) nbr_fetch<K>(pts, tk, xyz);
    }
  } else {
    const unsigned keep_mask = ~((1u << key_bits_for(g.n)) - 1u);
    KeyList<K + 1> L;
    keys_clear<K + 1>(L);
    int len = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) len = max(len, re[i] - rs[i]);
    if constexpr (NR == 1) {
      // PIECE walk (LPQ = 16).  The query's candidates -- its rows one after the other, T records -- are cut into 16-byte
      // pieces (piece p: record p >> 1, half p & 1) and piece t * 64 + u * 16 + sub is loaded by lane `sub` in instruction
      // u of trip t: the sixteen lanes of one load instruction cover 256 contiguous bytes of a row (a row boundary starts
      // a new run), where a row-owner lane's eight instructions per trip (four records x two halves) each looked the
      // same one or two lines up again.  A trip is 32 records; the lane pair (2i, 2i + 1) joins the halves of its record
      // and the even lane inserts it -- same distance, same index, same key as a row-owner walk would insert, and the
      // kept list is a sorted set of distinct keys, so the order of insertion does not show.
      //
      // Row table: the exclusive prefix of the nine row lengths by four row_shr steps inside the sixteen-lane DPP row (no
      // LDS, no barrier); lane k keeps (prefix, start - prefix) of row k, the lanes behind the rows hold prefix = T.  A
      // piece finds its row by a BINARY SEARCH BY SHUFFLE over the sixteen prefixes (four steps, then one shuffle for the
      // offset): two registers live across the loop and the kernel's 84 VGPRs unchanged, where nine broadcasts of the
      // pairs to every lane held seventeen (90 VGPRs) for the same kernel time (CHANGELOG).
      const int ln = re[0] - rs[0];   // (0 on the lanes without a row)
      int inc = ln;
      inc += row_dpp<0x111>(inc);   // row_shr:1
      inc += row_dpp<0x112>(inc);   // row_shr:2
      inc += row_dpp<0x114>(inc);   // row_shr:4
      inc += row_dpp<0x118>(inc);   // row_shr:8
      const int pre_own = inc - ln, off_own = rs[0] - pre_own;
      int T = row_dpp<0x15F>(inc);   // row_newbcast:15 -- the query's candidate count
#ifdef TLOAM_K1_DBG_NOWALK  // timing experiment only
      T = 0;
#endif
      constexpr int kPc = 4;   // load instructions per trip: 4 x 16 pieces = 32 records
      const bool even = (sub & 1) == 0;
      const char* const half0 = reinterpret_cast<const char*>(pts.p) + (sub & 1) * 16;
      // (T is the same on the sixteen lanes of a query; the wave runs the longest of its queries' trip counts)
      for (int b = 0; b < T; b += 8 * kPc) {
        int jp[kPc];
        bool vp[kPc];
        double2 c[kPc];
#pragma unroll
        for (int u = 0; u < kPc; ++u) {
          const int rec = b + u * 8 + (sub >> 1);   // the record of piece t * 64 + u * 16 + sub, t = b / 32
          int row = 0;   // the last row that starts at or before it (empty rows are stepped over; past the end: lane 15)
#pragma unroll
          for (int st = 8; st >= 1; st >>= 1) row += (__shfl(pre_own, row + st, 16) <= rec) ? st : 0;
          const int o = __shfl(off_own, row, 16);   // (by every lane, outside the select below: a shuffle reads active lanes only)
          vp[u] = rec < T;
          jp[u] = vp[u] ? rec + o : 0;   // a piece past the end loads record 0
        }
#pragma unroll
        for (int u = 0; u < kPc; ++u) c[u] = *reinterpret_cast<const double2*>(half0 + (size_t)jp[u] * sizeof(double4));
#pragma unroll
        for (int u = 0; u < kPc; ++u) {
          // the odd lane holds (z, index): its z goes to the even lane (quad_perm [1,0,3,2]), which holds (x, y)
          const double z = __hiloint2double(row_dpp<0xB1>(__double2hiint(c[u].x)), row_dpp<0xB1>(__double2loint(c[u].x)));
          key_insert<K + 1>(L, key_pack(sqdist(pw.x, pw.y, pw.z, c[u].x, c[u].y, z), jp[u], keep_mask, vp[u] && even));
        }
      }
    } else {
      // ROW-OWNER walk (LPQ = 4: three rows per lane).  kU steps per trip: candidates s .. s + kU - 1 of each of this
      // lane's rows are requested together (one record round trip per trip, so the trip carries as many as the rows allow)
      constexpr int kU = 2;
#ifdef TLOAM_K1_DBG_NOWALK  // timing experiment only
      len = 0;
#endif
      for (int s = 0; s < len; s += kU) {
        double4 c[kU][NR];
#pragma unroll
        for (int u = 0; u < kU; ++u)
#pragma unroll
          for (int i = 0; i < NR; ++i) c[u][i] = pts.p[(rs[i] + s + u < re[i]) ? rs[i] + s + u : 0];
#pragma unroll
        for (int u = 0; u < kU; ++u)
#pragma unroll
          for (int i = 0; i < NR; ++i) {
            const bool v = rs[i] + s + u < re[i];
            key_insert<K + 1>(L, key_pack(sqdist(pw.x, pw.y, pw.z, c[u][i].x, c[u][i].y, c[u][i].z), rs[i] + s + u, keep_mask, v));
          }
      }
    }
    TL_K1_STAMP(3)
    // merge across the quad: after xor-1 and xor-2 every lane holds the global list (the lanes' candidate
    // sets are disjoint, +inf entries fall through)
#ifndef TLOAM_K1_DBG_NOMERGE  // timing experiment only: without the cross-lane merge
#pragma unroll
    for (int x = 1; x < LPQ; x <<= 1) {
      double ok[K + 1];
#pragma unroll
      for (int m = 0; m < K + 1; ++m) ok[m] = __shfl_xor(L.k[m], x, 64);
#pragma unroll
      for (int m = 0; m < K + 1; ++m) key_insert<K + 1>(L, ok[m]);
    }
#endif
    TL_K1_STAMP(4)
    if (!keys_ambiguous<K + 1>(L, keep_mask)) {  // (the same verdict on all lanes of the quad)
      keys_unpack<K, K + 1>(L, pts, pw.x, pw.y, pw.z, keep_mask, tk, xyz);
      TL_K1_STAMP(5)
    } else {  // redo with the exact (d, original index) order (rare: it stays a row-owner loop at LPQ = 16 too, a record per lane and trip)
      for (int s = 0; s < len; ++s) {
        double4 c[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) c[i] = pts.p[(rs[i] + s < re[i]) ? rs[i] + s : 0];
#pragma unroll
        for (int i = 0; i < NR; ++i)
          if (rs[i] + s < re[i])
            topk_insert<K, PtsGlobal>(tk, pts, sqdist(pw.x, pw.y, pw.z, c[i].x, c[i].y, c[i].z), rs[i] + s);
      }
#pragma unroll
      for (int x = 1; x < LPQ; x <<= 1) {
        double od[K];
        int oj[K];
#pragma unroll
        for (int m = 0; m < K; ++m) { od[m] = __shfl_xor(tk.d[m], x, 64); oj[m] = __shfl_xor(tk.j[m], x, 64); }
#pragma unroll
        for (int m = 0; m < K; ++m)
          if (oj[m] >= 0) topk_insert<K, PtsGlobal>(tk, pts, od[m], oj[m]);
      }
      if (xyz) nbr_fetch<K>(pts, tk, xyz);
    }
  }
}

}  // namespace tl
