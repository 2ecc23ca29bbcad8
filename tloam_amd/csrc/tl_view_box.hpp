// tl_view_box.hpp -- the host arithmetic of the closed map's view gain (tl_api_view.hip): the side, the bits,
// the words and the bytes of a view's bit window, which of the two forms takes it, how many windows the global form holds at once
// and in how many chunks the views go, how many blocks a launch has, and every refusal, no product formed before it is checked
// (tl_tile_box.hpp's make_box is the model).  No HIP and no context in here, so that a stand-alone program can drive it under
// the host sanitizers (tests/host/view_box_main.cpp).
#pragma once

#include <math.h>
#include <stdint.h>

namespace tlv {

constexpr int kFormAuto = 0, kFormLds = 1, kFormGlobal = 2;
constexpr int64_t kMostW = ((int64_t)1 << 20) - 1;        // S = 2 W + 1 < 2^21: S^3 < 2^63 is formed without overflow
constexpr uint64_t kMostBlocks = 0x7FFFFFFFull;           // a launch's grid
constexpr uint64_t kMostInt64 = 0x7FFFFFFFFFFFFFFFull;

struct Window {
  int64_t W;        // cells each way from the origin's cell: (int) ceil(max_range / voxel) + 1
  int64_t S;        // the side, 2 W + 1
  uint64_t bits;    // S^3
  uint64_t words;   // ceil(bits / 32)
  uint64_t bytes;   // 4 * words
};

// The window of a view under max_range and voxel (both > 0 and finite), the quotient and its ceiling formed in double.  false:
// an argument out of that range or a side beyond kMostW; *out is then not to be used.
inline bool make_window(double max_range, double voxel, Window* out) {
  if (!(max_range > 0.0) || !(voxel > 0.0) || !isfinite(max_range) || !isfinite(voxel)) return false;
  const double up = ceil(max_range / voxel);
  if (!(up >= 1.0) || !(up < (double)kMostW)) return false;   // (a quotient that underflows to 0 has ceil 0: up >= 1 refuses it)
  out->W = (int64_t)up + 1;
  out->S = 2 * out->W + 1;                                     // < 2^21
  out->bits = (uint64_t)out->S * (uint64_t)out->S * (uint64_t)out->S;
  out->words = (out->bits + 31u) / 32u;
  out->bytes = 4u * out->words;
  return true;
}

// Which form runs: `form` 0 takes the LDS form when the window's bytes are at most lds_bytes, else the global one; 1 is the LDS
// form and false when the window does not fit; 2 the global form.  false also for a form or an lds_bytes out of range.
inline bool choose_form(int form, uint64_t window_bytes, int64_t lds_bytes, int* ran) {
  if (lds_bytes < 0 || form < kFormAuto || form > kFormGlobal) return false;
  const bool fits = window_bytes <= (uint64_t)lds_bytes;
  if (form == kFormLds && !fits) return false;
  *ran = form == kFormGlobal || !fits ? kFormGlobal : kFormLds;
  return true;
}

// The rays of a call: views >= 1, rays >= 1, their product within int64 (checked by division), and the two uploads' bytes
// (128 a pose, 24 an end) within int64 too.
inline bool ray_count(uint64_t views, uint64_t rays, uint64_t* total) {
  if (views == 0 || rays == 0) return false;
  if (views > kMostInt64 / 128u || rays > kMostInt64 / 24u) return false;
  if (rays > kMostInt64 / views) return false;
  *total = views * rays;
  return true;
}

// The global form's chunks: as many windows at once as max_bytes holds, at most `views` (>= 1) and at most a launch's grid.
// false: max_bytes < 4, or not even one window fits.
inline bool make_chunks(uint64_t views, uint64_t window_bytes, int64_t max_bytes, uint64_t* per_chunk, uint64_t* chunks) {
  if (views == 0 || window_bytes == 0 || max_bytes < 4) return false;
  uint64_t per = (uint64_t)max_bytes / window_bytes;
  if (per == 0) return false;
  if (per > views) per = views;
  if (per > kMostBlocks) per = kMostBlocks;
  *per_chunk = per;
  *chunks = views / per + (views % per ? 1u : 0u);
  return true;
}

// The blocks of the global form's ray launch: views_in_chunk * blocks_per_view, held to a launch's grid by lowering
// blocks_per_view (>= 1 stays: views_in_chunk <= kMostBlocks by make_chunks).  want: what the caller asks for, >= 1.
inline uint64_t blocks_per_view(uint64_t views_in_chunk, uint64_t want) {
  if (want < 1) want = 1;
  const uint64_t most = views_in_chunk ? kMostBlocks / views_in_chunk : 1u;
  return want > most ? (most ? most : 1u) : want;
}

}  // namespace tlv
