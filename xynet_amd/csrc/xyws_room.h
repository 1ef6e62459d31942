// xyws_room.h — internal: what the kernels that walk a room's members share
// (xyws_broadcast.hip: the wire build and the fan-out; xyws_backlog.hip: the
// backlog fold and the delivery): how a member and its gate follow from its
// reassembly and reply rows (load_member), which of its stored records is
// deliverable behind that gate and how long its frame is (frame_of;
// include/xyws.h, xyws_broadcast_streams 2. and 3.), the workgroup scan that
// places members, and the geometry of the two fan-out launches. Each is stated
// once here: the gate rule is load_member's and nobody else's. The rows are
// read through xyws_rows.h, which names their words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_frameops.h"
#include "xyws_rows.h"

#define BC_WAVE 64u
#define BC_WIRE_THREADS 1024u  // the wire build: sixteen waves, the one workgroup a room gets
// the fan-out and the backlog delivery (xyws_host.h: fanout_grid)
#define BC_THREADS 256u     // four waves
#define BC_LINE 16u         // bytes a thread writes per copy step
#define BC_STEP (BC_LINE * BC_THREADS)  // bytes a workgroup writes per step
#define BC_GRID_CAP 8192u   // rooms / connections per launch in x; further ones are grid-strided
#define BC_BLOCKS_AIM 4096u // workgroups wanted in flight (256 CUs x 16)
#define BC_SLICES_MAX 256u  // at most this many workgroups share one connection

namespace xyws_internal {

// What the wire build keeps of a member: gate = records with first_frame
// below it can be delivered (0: none; XYWS_NPOS: no close in this sweep).
struct member {
  uint64_t msgs, gate, out, out_cap, head, head_len;
  uint32_t stored;
};

// Member ci (< n of the caller's tables) from its reassembly entry and row,
// its broadcast entry and, where it names one, its reply row. The gate:
// nothing after a reassembly or reply overflow or a close in an earlier sweep,
// else the frames before the first close of this sweep. receiver: it takes
// the room's wire (neither closed nor overflowed); over_cap: the sweep found
// more messages than msg_cap holds.
XYWS_DEV void load_member(const xyws_reasm_conn* reasm, const xyws_reasm_result* rres, const xyws_bcast_conn* bconns,
                          uint64_t ci, member& m, bool& receiver, bool& over_cap) {
  const xyws_rows::reasm_conn_row aq = xyws_rows::load_reasm_conn<false>(reasm + ci);
  const xyws_rows::reasm_result_row ar = xyws_rows::load_reasm_result<false>(rres + ci);
  const xyws_rows::bcast_conn_row bq = xyws_rows::load_bcast_conn<false>(bconns + ci);
  m.out = aq.out;
  m.out_cap = aq.out_cap;
  m.msgs = aq.msgs;
  const uint64_t msg_cap = aq.msg_cap, nmsgs = ar.nmsgs;
  const uint32_t rst = ar.counts.status;
  const uint64_t kept = nmsgs < msg_cap ? nmsgs : msg_cap;
  m.stored = kept < 0xFFFFFFFFull ? (uint32_t)kept : 0xFFFFFFFFu;  // (the counts are 32 bits)
  over_cap = nmsgs > msg_cap;
  m.head = bq.head;
  m.head_len = bq.head_len;
  m.gate = (rst & XYWS_RSM_OVERFLOW) ? 0 : XYWS_NPOS;
  receiver = true;
  if (bq.reply) {
    const xyws_rows::reply_result_row rp = xyws_rows::load_reply_result<false>((const xyws_reply_result*)bq.reply);
    const uint64_t fc = rp.first_close;
    const uint32_t pst = rp.status;
    if (pst & (XYWS_RPL_CLOSED | XYWS_RPL_OVERFLOW)) receiver = false;
    if ((pst & XYWS_RPL_OVERFLOW) || ((pst & XYWS_RPL_CLOSED) && fc == XYWS_NPOS)) m.gate = 0;
    else if (fc != XYWS_NPOS && m.gate) m.gate = fc;
  }
}

// One stored record (rec) of a member: deliverable or not;
// if so its frame: header words hw, header length h, message at out + off,
// length len.
struct frame_info {
  uint64_t off, len;
  uint32_t hw[4], h;
};
XYWS_DEV bool frame_of(const xyws_message* rec, const member& m, uint32_t flags, uint32_t enc_opts, frame_info& f) {
  const xyws_rows::message_row r = xyws_rows::load_message<false>(rec);
  const xyws_rows::message_meta meta = xyws_rows::unpack_message_meta(r.meta);
  const uint64_t first = r.first_frame, off = r.out_off, len = r.length;
  const uint32_t st = meta.status, op = meta.opcode & XYWS_FLAG_OP_MASK;
  if (!(st & XYWS_MSG_COMPLETE) || (st & (XYWS_MSG_CONTINUED | XYWS_MSG_TRUNCATED | XYWS_MSG_UTF8_BAD))) return false;
  if (!in_range(off, len, m.out_cap)) return false;  // (nothing outside [out, out + out_cap) is read)
  if (m.gate != XYWS_NPOS && first >= m.gate) return false;
  f.off = off;
  f.len = len;
  const uint32_t fl = (enc_opts & XYWS_ENC_FRAME_OPCODE) ? (flags & ~(uint32_t)XYWS_FLAG_OP_MASK) | op : flags;
  f.h = build_header(fl, m.head_len + len, false, 0, f.hw);
  return true;
}

// Inclusive scan of v over a workgroup of WAVES waves (s_w: one slot per wave); total: the sum.
template <uint32_t WAVES = BC_WIRE_THREADS / BC_WAVE>
XYWS_DEV uint64_t block_scan(uint64_t v, uint32_t tid, uint64_t* s_w, uint64_t& total) {
  const uint32_t lane = tid & (BC_WAVE - 1u), wave = tid / BC_WAVE;
  const uint64_t incl = wave_scan64(v, lane);
  if (lane == BC_WAVE - 1u) s_w[wave] = incl;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < WAVES; w++) {
    const uint64_t x = s_w[w];
    if (w < wave) before += x;
    all += x;
  }
  total = all;
  __syncthreads();  // (s_w is reused)
  return incl + before;
}

}  // namespace xyws_internal
