// xyws_frameops.h — internal: the per-frame rules that the kernels over a
// decoded frame table share (xyws_frames.hip: xyws_encode_frames and
// xyws_classify_frames; xyws_reply.hip: xyws_reply_streams). Each rule is
// stated once here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xyws.h"
#include "xyws_device.h"

namespace xyws_internal {

// ---------------------------------------------------------------- header build
// detail::websocket_frame_header_builder (:136-175) into four little-endian
// words (byte i = w[i/4] >> 8*(i%4)); returns H. The key word kw (wire bytes,
// little-endian) is written only when has_key, as the builder copies the
// key only for a non-null mask (:168-173). Register-only (no byte array).
__host__ __device__ inline uint32_t build_header(uint32_t flags, uint64_t len, bool has_key, uint32_t kw,
                                                 uint32_t w[4]) {
  const uint32_t b0 = ((flags & XYWS_FLAG_FIN) ? 0x80u : 0u) | (flags & XYWS_FLAG_OP_MASK);
  uint32_t b1 = (flags & XYWS_FLAG_HAS_MASK) ? 0x80u : 0u;
  const bool masked = (flags & XYWS_FLAG_HAS_MASK) != 0;
  const uint32_t k = has_key ? kw : 0u;
  w[0] = w[1] = w[2] = w[3] = 0;
  uint32_t h;
  if (len < 126u) {
    b1 |= (uint32_t)len;
    w[0] = b0 | (b1 << 8);
    if (masked) { w[0] |= k << 16; w[1] = k >> 16; }
    h = 2;
  } else if (len <= 0xFFFFu) {
    b1 |= 126u;
    w[0] = b0 | (b1 << 8) | ((uint32_t)(len >> 8) << 16) | ((uint32_t)(len & 0xFFu) << 24);
    if (masked) w[1] = k;
    h = 4;
  } else {
    b1 |= 127u;
    // bytes 2..9: the length big-endian = the little-endian bytes of bswap64(len)
    uint64_t be = 0;
    for (int i = 0; i < 8; i++) be |= ((len >> (8 * i)) & 0xFFull) << (56 - 8 * i);
    w[0] = b0 | (b1 << 8) | ((uint32_t)(be & 0xFFFFu) << 16);
    w[1] = (uint32_t)(be >> 16);
    w[2] = (uint32_t)(be >> 48);
    if (masked) { w[2] |= k << 16; w[3] = k >> 16; }
    h = 10;
  }
  return masked ? h + 4 : h;
}

// The flags of the reply to a frame with flags `fflags`: the caller's, or with
// XYWS_ENC_FRAME_OPCODE the frame's own opcode and FIN (a ping answered as a
// pong) plus the caller's HAS_MASK bit.
__host__ __device__ inline uint32_t reply_flags_of(uint32_t flags, uint32_t enc_opts, uint32_t fflags) {
  if (!(enc_opts & XYWS_ENC_FRAME_OPCODE)) return flags;
  uint32_t op = fflags & XYWS_FLAG_OP_MASK;
  if (op == XYWS_FLAG_OP_PING) op = XYWS_FLAG_OP_PONG;
  return op | (fflags & XYWS_FLAG_FIN) | (flags & XYWS_FLAG_HAS_MASK);
}

// ---------------------------------------------------------------- close policy
// websocket_check_parser_result (example/include/common/websocket.h:81-108)
// for one frame: the verdict xyws_classify_frames documents. `src` (any
// pointer to bytes) is read only for a close frame's status code, and only
// inside [0, src_len).
template <class Src>
XYWS_DEV xyws_verdict classify_frame(uint32_t fflags, uint32_t fstatus, uint64_t payload_off, uint64_t payload_len,
                                     Src src, uint64_t src_len, uint64_t max_payload, uint32_t policy) {
  const uint32_t op = fflags & XYWS_FLAG_OP_MASK;
  xyws_verdict v;
  v.close_code = 0;
  v.peer_code = 0;
  v.action = op == XYWS_FLAG_OP_PING ? XYWS_ACT_PING : op == XYWS_FLAG_OP_PONG ? XYWS_ACT_PONG : XYWS_ACT_DATA;
  v.reserved[0] = v.reserved[1] = v.reserved[2] = 0;
  const bool proto = (fstatus & (XYWS_ST_RSV | XYWS_ST_RESERVED_OPCODE | XYWS_ST_BAD_CONTROL)) != 0;
  uint16_t code = 0;
  if ((policy & XYWS_POL_STRICT) && proto) code = 1002;
  else if (op == XYWS_FLAG_OP_CLOSE || ((policy & XYWS_POL_REFERENCE) && (op & 8u)))
    code = 1000;  // (websocket.h:87-90: the opcode compared exactly, or its bit 3 as the reference tests it)
  else if (!(fflags & XYWS_FLAG_FIN) && !(policy & XYWS_POL_FRAGMENTS)) code = 1003;
  else if (!(fflags & XYWS_FLAG_HAS_MASK) && !(policy & XYWS_POL_UNMASKED)) code = 1008;
  else if (payload_len > max_payload) code = 1009;
  if (op == XYWS_FLAG_OP_CLOSE) {
    v.action = XYWS_ACT_CLOSE;
    const uint64_t p = payload_off;
    v.peer_code = 1005;  // (RFC 6455 7.4.1: no status code present)
    if (payload_len >= 2 && p < src_len && src_len - p >= 2) v.peer_code = (uint16_t)((src[p] << 8) | src[p + 1]);
  }
  if (code) {
    v.close_code = code;
    v.action = XYWS_ACT_CLOSE;
  }
  return v;
}

// ---------------------------------------------------------------- UTF-8 rules
// (RFC 3629, shared by k_utf8 / k_rs_carry in xyws_frames.hip and by
// k_reasm_streams in xyws_reasm_streams.hip)
// Bytes of the sequence a lead byte announces (0: not a lead).
XYWS_DEV uint32_t lead_len(uint32_t c) { return c >= 0xF0u ? 4u : c >= 0xE0u ? 3u : c >= 0xC0u ? 2u : 0u; }
// The second-byte rules of lead c0: overlongs (E0, F0), surrogates (ED), code
// points above U+10FFFF (F4).
XYWS_DEV bool utf8_second_bad(uint32_t c0, uint32_t c1) {
  return (c0 == 0xE0u && c1 < 0xA0u) || (c0 == 0xEDu && c1 > 0x9Fu) || (c0 == 0xF0u && c1 < 0x90u) ||
         (c0 == 0xF4u && c1 > 0x8Fu);
}
// A carried UTF-8 tail as one word: its 0..3 bytes in bits 0..23, their
// count in bits 24..31 (0: none). tail_prev: the byte `back` (>= 1) before
// the message's first byte in this call, or 0x100 when the tail is shorter.
XYWS_DEV uint32_t tail_word(const xyws_msg_carry* mc) {
  if (!mc || mc->opcode != XYWS_FLAG_OP_TEXT || !mc->utf8_len || mc->utf8_len > 3) return 0;
  return (uint32_t)mc->utf8[0] | ((uint32_t)mc->utf8[1] << 8) | ((uint32_t)mc->utf8[2] << 16) |
         ((uint32_t)mc->utf8_len << 24);
}
XYWS_DEV uint32_t tail_prev(uint32_t tw, uint32_t back) {
  const uint32_t tl = tw >> 24;
  if (back > tl) return 0x100u;
  return (tw >> (8u * (tl - back))) & 0xFFu;
}

// ---------------------------------------------------------------- message records
// A stored record's bytes [off, off + len) lie in [0, out_cap): nothing outside
// a connection's out area is read (the room kernels' frame_of, xyws_room.h;
// xyws_hold.hip).
XYWS_DEV bool in_range(uint64_t off, uint64_t len, uint64_t out_cap) { return off <= out_cap && len <= out_cap - off; }

// ---------------------------------------------------------------- lane moves
// (the 16-byte line loads and stores of the copy phases: xyws_lines.h)
XYWS_DEV uint64_t shfl64(uint64_t v, uint32_t src) {
  return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, (int)src) |
         ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src) << 32);
}
XYWS_DEV uint64_t shfl_up64(uint64_t v, uint32_t d) {
  return (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)v, d) |
         ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d) << 32);
}
// Inclusive scan of v across the 64 lanes of a wave.
XYWS_DEV uint64_t wave_scan64(uint64_t v, uint32_t lane) {
  uint64_t incl = v;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint64_t o = shfl_up64(incl, d);
    if (lane >= d) incl += o;
  }
  return incl;
}

}  // namespace xyws_internal
