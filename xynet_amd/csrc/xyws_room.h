// xyws_room.h — internal: what the kernels that walk a room's members share
// (xyws_broadcast.hip: the wire build; xyws_backlog.hip: the backlog fold):
// which of a member's stored records is deliverable behind a given gate and
// how long its frame is (include/xyws.h, xyws_broadcast_streams 2. and 3.),
// and the workgroup scan both use to place members. The record test and the
// frame size are stated once here; how a member's gate follows from its
// reassembly and reply rows is written in each of the two kernels (the wire
// build's lines were left as they were), and a difference between them shows
// as XYWS_BL_MISMATCH, never as a wrong copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_frameops.h"

#define BC_WAVE 64u
#define BC_WIRE_THREADS 1024u  // the wire build: sixteen waves, the one workgroup a room gets

namespace xyws_internal {

// What the wire build keeps of a member: gate = records with first_frame
// below it can be delivered (0: none; XYWS_NPOS: no close in this sweep).
struct member {
  uint64_t msgs, gate, out, out_cap, head, head_len;
  uint32_t stored;
};

// One stored record (its five words at rec) of a member: deliverable or not;
// if so its frame: header words hw, header length h, message at out + off,
// length len.
struct frame_info {
  uint64_t off, len;
  uint32_t hw[4], h;
};
XYWS_DEV bool frame_of(const g_u64* rec, const member& m, uint32_t flags, uint32_t enc_opts, frame_info& f) {
  const uint64_t first = rec[0], off = rec[2], len = rec[3], w4 = rec[4];
  const uint32_t st = (uint32_t)w4, op = (uint32_t)(w4 >> 32) & XYWS_FLAG_OP_MASK;
  if (!(st & XYWS_MSG_COMPLETE) || (st & (XYWS_MSG_CONTINUED | XYWS_MSG_TRUNCATED | XYWS_MSG_UTF8_BAD))) return false;
  if (off > m.out_cap || len > m.out_cap - off) return false;  // (nothing outside [out, out + out_cap) is read)
  if (m.gate != XYWS_NPOS && first >= m.gate) return false;
  f.off = off;
  f.len = len;
  const uint32_t fl = (enc_opts & XYWS_ENC_FRAME_OPCODE) ? (flags & ~(uint32_t)XYWS_FLAG_OP_MASK) | op : flags;
  f.h = build_header(fl, m.head_len + len, false, 0, f.hw);
  return true;
}

// Inclusive scan of v over the workgroup (s_w: one slot per wave); total: the sum.
XYWS_DEV uint64_t block_scan(uint64_t v, uint32_t tid, uint64_t* s_w, uint64_t& total) {
  const uint32_t lane = tid & (BC_WAVE - 1u), wave = tid / BC_WAVE;
  uint64_t incl = v;
#pragma unroll
  for (uint32_t d = 1; d < BC_WAVE; d <<= 1) {
    const uint64_t o = shfl_up64(incl, d);
    if (lane >= d) incl += o;
  }
  if (lane == BC_WAVE - 1u) s_w[wave] = incl;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < BC_WIRE_THREADS / BC_WAVE; w++) {
    const uint64_t x = s_w[w];
    if (w < wave) before += x;
    all += x;
  }
  total = all;
  __syncthreads();  // (s_w is reused)
  return incl + before;
}

}  // namespace xyws_internal
