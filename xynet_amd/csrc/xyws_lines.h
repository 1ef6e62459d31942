// xyws_lines.h — internal: the 16-byte line copy that the per-connection and
// per-room kernels share (xyws_reply.hip, xyws_reasm_streams.hip,
// xyws_broadcast.hip, xyws_hold.hip, xyws_backlog.hip). Each rule is stated
// once here.
//
// A destination range is addressed from a 16-byte-aligned base at or below its
// first byte: positions [P0, P1), cut at a capacity limit where there is one.
// A thread takes one destination-aligned line [A, A + 16) per step, composes
// the line's bytes in registers at their line offsets (source bytes: one or
// two aligned 16-byte loads funnelled to the byte offset), and ends the line
// with put_line: one 16-byte store where the whole line is the range's and
// lies inside the capacity, byte stores of its own bytes otherwise. A send
// slab's neighbours share the first and last line of every range, so nothing
// outside the range is ever written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xyws_device.h"

namespace xyws_internal {

// ---------------------------------------------------------------- loads
XYWS_DEV bytes16 line_of(const g_u8* aligned) {
  const u32x4 x = *reinterpret_cast<const g_u32x4*>(aligned);
  return bytes16{(uint64_t)x.x | ((uint64_t)x.y << 32), (uint64_t)x.z | ((uint64_t)x.w << 32)};
}
// The nb (1..16) bytes at address g, in the low bytes of the result (the bytes
// above them are not defined). Only the 16-byte lines that hold one of the nb
// bytes are loaded.
XYWS_DEV bytes16 load_bytes(uint64_t g, uint32_t nb) {
  const g_u8* const a = (const g_u8*)(g & ~15ull);
  const uint32_t sh = (uint32_t)(g & 15u);
  bytes16 v = shr_bytes(line_of(a), sh);
  if (sh + nb > 16) {  // (sh >= 1 here)
    const bytes16 y = shl_bytes(line_of(a + 16), 16 - sh);
    v.lo |= y.lo;
    v.hi |= y.hi;
  }
  return v;
}

// ---------------------------------------------------------------- composing a line
// The first nb bytes of v to line offset a of acc; a and the running position
// q move past them.
XYWS_DEV void add_bytes(bytes16& acc, uint32_t& a, uint64_t& q, bytes16 v, uint32_t nb) {
  const bytes16 p = shl_bytes(low_bytes(v, nb), a);
  acc.lo |= p.lo;
  acc.hi |= p.hi;
  a += nb;
  q += nb;
}

// The last of the n_items items whose start s_off[i] is at or before q: the
// item that holds byte q (s_off ascending, s_off[0] <= q).
XYWS_DEV uint32_t item_at(const uint64_t* s_off, uint32_t n_items, uint64_t q) {
  uint32_t i = 0, hi = n_items;
  while (hi - i > 1) {
    const uint32_t m = (i + hi) >> 1;
    if (s_off[m] <= q) i = m;
    else hi = m;
  }
  return i;
}

// ---------------------------------------------------------------- stores
XYWS_DEV void store_line(g_u8* base, uint64_t A, bytes16 v) {
  *reinterpret_cast<g_u32x4*>(base + A) =
      u32x4{(uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32)};
}
// Bytes [s, we) of the line at A, byte by byte (v holds the line's bytes at
// their line offsets; A <= s <= we <= A + 16). The loop counts the line offset
// in 32 bits: with a 64-bit position every caller needs more registers (the
// resource table in DESIGN.md 4.7).
XYWS_DEV void store_edge(g_u8* base, uint64_t A, uint64_t s, uint64_t we, bytes16 v) {
#pragma unroll 1
  for (uint32_t b = (uint32_t)(s - A), be = (uint32_t)(we - A); b < be; b++)
    base[A + b] = (uint8_t)(b < 8 ? v.lo >> (8u * b) : v.hi >> (8u * (b - 8)));
}
// Ends the line at A, of which [s, e) are the range's bytes (v holds them at
// their line offsets) and [lo, lim) may be written: a whole store when the
// line is all the range's and inside [lo, lim), else bytes [s, min(e, lim)).
XYWS_DEV void put_line(g_u8* base, uint64_t A, uint64_t s, uint64_t e, uint64_t lo, uint64_t lim, bytes16 v) {
  if (s == A && e == A + 16 && A >= lo && A + 16 <= lim) store_line(base, A, v);
  else store_edge(base, A, s, e < lim ? e : lim, v);
}

// ---------------------------------------------------------------- the plain copy
// Source bytes src[0, wl - P0) to positions [P0, wl) from dst_base (wl > P0;
// the caller has cut wl at its capacity and checked both ranges). Thread t
// takes the lines A = align16(P0) + first + 16 t, A + stride, .. below wl.
// Whole lines keep a path of their own, without the shift to line offsets.
// Callers: the backlog delivery and the hold's copies (the fan-out keeps the
// same loop in its kernel).
XYWS_DEV void copy_span(g_u8* dst_base, uint64_t P0, uint64_t wl, uint64_t src, uint64_t first, uint64_t stride,
                        uint32_t t) {
  for (uint64_t A0 = (P0 & ~15ull) + first; A0 < wl; A0 += stride) {
    const uint64_t A = A0 + 16u * t;
    if (A >= wl) break;
    if (A >= P0 && A + 16 <= wl) {  // a whole line inside the range: source bytes A - P0 .., no shift
      store_line(dst_base, A, load_bytes(src + (A - P0), 16));
    } else {  // the range's first or last line: its own bytes only
      const uint64_t s = A > P0 ? A : P0, e = A + 16 < wl ? A + 16 : wl;
      put_line(dst_base, A, s, e, P0, wl, shl_bytes(load_bytes(src + (s - P0), (uint32_t)(e - s)), (uint32_t)(s - A)));
    }
  }
}

}  // namespace xyws_internal
