// xyws_outbox.hip — xyws_outbox_streams: the send bytes of a whole sweep packed
// into one buffer, with the ordered list of who sends or closes and a summary
// (the reference drains m_write_msgs into m_socket.send once per connection,
// example/websocket/websocket_chat.cpp:148-175, and closes through
// websocket_send_close, example/include/common/websocket.h:70-79). The
// semantics are stated in include/xyws.h; this is how they are computed. Every
// table row is read and written through xyws_rows.h, which names its words.
//
// Three launches, dev_scratch the hand-over between them. No workgroup waits
// for another inside a launch, nothing spins, there are no atomics.
//
// k_outbox_plan: one thread per connection, one workgroup per tile of OB_TILE.
// The thread loads its row and the result rows it names, computes len,
// full_len and the flags; workgroup scans (wave scans by shuffles, wave totals
// through LDS: block_scan, xyws_room.h) give its entry index and slot offset
// inside the tile. It keeps a plan record per connection and the tile's sums.
//
// k_outbox_scan: one workgroup. It scans the tile sums in place into each
// tile's first entry index and first slot offset, looping for more tiles than
// threads, and writes the summary. Slot ends ascend with the offsets, so the
// packed slots are a prefix of those with bytes: the tiles before the first
// one whose end lies above the capacity are packed whole, those behind it are
// deferred whole, and that one tile's records are read again, one per thread.
//
// k_outbox_pack: blockIdx.x strides over the connections, blockIdx.y over
// OB_STEP-byte chunks of a slot, chunk c to workgroup c mod gridDim.y (the
// host knows no length: the grid comes from n alone, as k_room_fanout's). The
// y == 0 workgroup writes the connection's entry. Slots begin at multiples of
// 16, so every store is one whole line (store_line, xyws_lines.h); the source
// side is load_bytes at any alignment, and low_bytes zeroes the pad of a
// slot's last line.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_lines.h"
#include "xyws_room.h"
#include "xyws_rows.h"

#define OB_WAVE BC_WAVE
#define OB_TILE 256u           // connections per tile of the plan pass: one per thread, four waves
#define OB_SCAN_THREADS 256u   // the scan pass: tiles per step of its one workgroup (16 waves spilled registers)
#define OB_THREADS 64u         // the pack pass: one wave per workgroup
#define OB_LINE 16u            // bytes a thread writes per copy step
#define OB_STEP (OB_LINE * OB_THREADS)  // bytes a workgroup writes per step
#define OB_GRID_CAP 4096u      // connections per launch in x; further ones are grid-strided
#define OB_BLOCKS_AIM 16384u   // one-wave workgroups wanted in flight (256 CUs x 64)
#define OB_SLICES_MAX 64u      // at most this many workgroups share one connection

static_assert(OB_SCAN_THREADS >= OB_TILE && OB_TILE % OB_WAVE == 0 && OB_SCAN_THREADS % OB_WAVE == 0,
              "the scan pass reads one tile's records with a thread each");

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

// dev_scratch: n plan records, then the tile sums.
// A plan record: what the pack pass needs of a connection. tag: the entry's
// flags, OB_LISTED, and from bit 32 the entry's index inside its tile.
struct ob_plan { uint64_t len, full_len, local_off, tag; };
// A tile's sums as the plan pass leaves them. The scan pass overwrites counts
// with the index of the tile's first entry and slot_bytes with its first
// slot's offset.
struct ob_tile {
  uint64_t counts;      // entries | entries with bytes << 32
  uint64_t slot_bytes;  // sum of align16(len)
  uint64_t send_bytes;  // sum of len
  uint64_t closes;      // n_close | n_truncated << 32
};
constexpr uint64_t OB_LISTED = 1ull << 31;
constexpr uint64_t OB_NO_TILE = ~0ull;

XYWS_DEV uint64_t align16(uint64_t v) { return (v + 15u) & ~15ull; }
// (scratch is device memory: global loads and stores, the records by their fields)
typedef XYWS_GLOBAL ob_plan g_plan;
typedef XYWS_GLOBAL ob_tile g_tile;

__host__ __device__ inline uint64_t tiles_for(uint64_t n) { return (n + OB_TILE - 1u) / OB_TILE; }

__global__ void __launch_bounds__(OB_TILE)
    k_outbox_plan(const xyws_outbox_conn* __restrict__ conns, uint64_t n, ob_plan* __restrict__ plan,
                  ob_tile* __restrict__ tiles) {
  __shared__ uint64_t s_w[OB_TILE / OB_WAVE];
  const uint32_t tid = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * OB_TILE + tid;
  uint64_t len = 0, full = 0;
  uint32_t flags = 0;
  if (i < n) {
    const rows::outbox_conn_row c = rows::load_outbox_conn<false>(conns + i);
    uint32_t rst = 0, ast = 0, resp_len = 0;
    uint64_t reply_len = 0;
    if (c.reply) {
      const rows::reply_result_row r = rows::load_reply_result<false>((const xyws_reply_result*)c.reply);
      reply_len = r.reply_len;
      rst = r.status;
    }
    if (c.accept) {
      const rows::accept_brief a = rows::load_accept_brief<false>((const xyws_accept_result*)c.accept);
      ast = a.status;
      resp_len = a.resp_len;
    }
    // rule 1: the last call of the sweep that wrote a row for it says what there is to send
    if (c.backlog) full = rows::load_backlog_send_len((const xyws_backlog_result*)c.backlog);
    else if (c.bcast) full = rows::load_bcast_result_own((const xyws_bcast_result*)c.bcast).send_len;
    else if (c.reply) full = reply_len;
    else if (ast & (XYWS_ACC_ACCEPTED | XYWS_ACC_REJECTED)) full = resp_len;
    len = full < c.out_cap ? full : c.out_cap;
    // rule 2
    if ((rst & XYWS_RPL_CLOSED) || (ast & XYWS_ACC_REJECTED)) flags |= XYWS_OB_CLOSE;
    if (rst & XYWS_RPL_OVERFLOW) flags |= XYWS_OB_OVERFLOW;
    if (full > c.out_cap) flags |= XYWS_OB_TRUNCATED;
  }
  const bool listed = len || flags;
  const uint64_t slot = align16(len);
  const uint64_t cnt = (listed ? 1ull : 0ull) | (len ? 1ull << 32 : 0ull);
  const uint64_t cls = (flags & XYWS_OB_CLOSE ? 1ull : 0ull) | (flags & XYWS_OB_TRUNCATED ? 1ull << 32 : 0ull);
  uint64_t t_cnt, t_slot, t_send, t_cls;
  const uint64_t incl_cnt = block_scan<OB_TILE / OB_WAVE>(cnt, tid, s_w, t_cnt);
  const uint64_t incl_slot = block_scan<OB_TILE / OB_WAVE>(slot, tid, s_w, t_slot);
  block_scan<OB_TILE / OB_WAVE>(len, tid, s_w, t_send);
  block_scan<OB_TILE / OB_WAVE>(cls, tid, s_w, t_cls);
  if (i < n) {
    g_plan* const p = (g_plan*)(plan + i);
    p->len = len;
    p->full_len = full;
    p->local_off = incl_slot - slot;
    p->tag = (uint64_t)flags | (listed ? OB_LISTED : 0ull) | (((incl_cnt - cnt) & 0xFFFFFFFFull) << 32);
  }
  if (tid == 0) {
    g_tile* const t = (g_tile*)(tiles + blockIdx.x);
    t->counts = t_cnt;
    t->slot_bytes = t_slot;
    t->send_bytes = t_send;
    t->closes = t_cls;
  }
}

__global__ void __launch_bounds__(OB_SCAN_THREADS)
    k_outbox_scan(const ob_plan* __restrict__ plan, uint64_t n, ob_tile* tiles, uint64_t n_tiles, uint64_t cap,
                  xyws_outbox_summary* __restrict__ summary) {
  __shared__ uint64_t s_w[OB_SCAN_THREADS / OB_WAVE];
  __shared__ uint64_t s_cut[2];  // the tile whose end is the first above cap, and its first slot's offset
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    s_cut[0] = OB_NO_TILE;
    s_cut[1] = 0;
  }
  uint64_t c_cnt = 0, c_slot = 0;            // the tiles so far (uniform)
  uint64_t a_send = 0, a_cls = 0, a_def = 0;  // this thread's tiles
  for (uint64_t base = 0; base < n_tiles; base += OB_SCAN_THREADS) {
    const uint64_t t = base + tid;
    uint64_t cnt = 0, slot = 0;
    if (t < n_tiles) {
      const g_tile* const w = (const g_tile*)(tiles + t);
      cnt = w->counts;
      slot = w->slot_bytes;
      a_send += w->send_bytes;
      a_cls += w->closes;
    }
    uint64_t t_cnt, t_slot;
    const uint64_t incl_cnt = block_scan<OB_SCAN_THREADS / OB_WAVE>(cnt, tid, s_w, t_cnt);
    const uint64_t incl_slot = block_scan<OB_SCAN_THREADS / OB_WAVE>(slot, tid, s_w, t_slot);
    if (t < n_tiles) {
      const uint64_t first = c_slot + (incl_slot - slot), end = c_slot + incl_slot;
      g_tile* const w = (g_tile*)(tiles + t);
      w->counts = (c_cnt + (incl_cnt - cnt)) & 0xFFFFFFFFull;
      w->slot_bytes = first;
      if (end > cap) {
        if (first <= cap) {  // (one tile at most: ends ascend, and a tile behind it begins above cap)
          s_cut[0] = t;
          s_cut[1] = first;
        } else {
          a_def += cnt >> 32;
        }
      }
    }
    c_cnt += t_cnt;
    c_slot += t_slot;
  }
  __syncthreads();
  // the one tile that is packed in part: its packed slots are the first ones
  const uint64_t cut = s_cut[0], cut_first = s_cut[1];
  uint64_t packed = 0;
  if (cut != OB_NO_TILE && tid < OB_TILE && cut * OB_TILE + tid < n) {
    const g_plan* const p = (const g_plan*)(plan + cut * OB_TILE + tid);
    const uint64_t len = p->len, local_off = p->local_off;
    if (len) {
      if (cut_first + local_off + align16(len) > cap) a_def++;
      else packed = align16(len);
    }
  }
  uint64_t t_send, t_cls, t_def, t_packed;
  block_scan<OB_SCAN_THREADS / OB_WAVE>(a_send, tid, s_w, t_send);
  block_scan<OB_SCAN_THREADS / OB_WAVE>(a_cls, tid, s_w, t_cls);
  block_scan<OB_SCAN_THREADS / OB_WAVE>(a_def, tid, s_w, t_def);
  block_scan<OB_SCAN_THREADS / OB_WAVE>(packed, tid, s_w, t_packed);
  if (tid < rows::OBS_WORDS) {
    const uint32_t n_close = (uint32_t)t_cls, n_trunc = (uint32_t)(t_cls >> 32), n_def = (uint32_t)t_def;
    uint64_t w[rows::OBS_WORDS];
    rows::pack_outbox_summary({c_cnt & 0xFFFFFFFFull, c_slot, cut == OB_NO_TILE ? c_slot : cut_first + t_packed, t_send,
                               {n_close, n_trunc},
                               {n_def, (n_def ? XYWS_OBS_DEFERRED : 0u) | (n_trunc ? XYWS_OBS_TRUNCATED : 0u)}},
                              w);
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < rows::OBS_WORDS; k++) mine = tid == k ? w[k] : mine;
    rows::store_outbox_summary_word(summary, tid, mine);
  }
}

__global__ void __launch_bounds__(OB_THREADS)
    k_outbox_pack(const xyws_outbox_conn* __restrict__ conns, uint64_t n, const ob_plan* __restrict__ plan,
                  const ob_tile* __restrict__ tiles, void* pack_mem, uint64_t cap, xyws_outbox_entry* entries) {
  const uint32_t tid = threadIdx.x;
  g_u8* const pack = (g_u8*)(uintptr_t)pack_mem;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const g_plan* const p = (const g_plan*)(plan + ci);
    const uint64_t tag = uniform64(p->tag);
    if (!(tag & OB_LISTED)) continue;
    const uint64_t len = uniform64(p->len), full = uniform64(p->full_len), local_off = uniform64(p->local_off);
    const g_tile* const t = (const g_tile*)(tiles + ci / OB_TILE);
    const uint64_t k = uniform64(t->counts) + (tag >> 32), off = uniform64(t->slot_bytes) + local_off;
    const bool deferred = len && off + align16(len) > cap;  // rule 4
    if (blockIdx.y == 0 && tid < rows::OBE_WORDS) {
      uint64_t w[rows::OBE_WORDS];
      const uint32_t flags = ((uint32_t)tag & (uint32_t)(OB_LISTED - 1u)) | (deferred ? XYWS_OB_DEFERRED : 0u);
      rows::pack_outbox_entry({{(uint32_t)ci, flags}, off, len, full}, w);
      uint64_t mine = 0;
#pragma unroll
      for (uint32_t j = 0; j < rows::OBE_WORDS; j++) mine = tid == j ? w[j] : mine;
      rows::store_outbox_entry_word(entries + k, tid, mine);
    }
    if (!len || deferred) continue;
    // slot byte q is out[q] for q < len and zero behind; line A of the slot is at off + A of the pack
    const uint64_t out = rows::load_outbox_out(conns + ci);
    for (uint64_t A0 = (uint64_t)blockIdx.y * OB_STEP; A0 < len; A0 += (uint64_t)gridDim.y * OB_STEP) {
      const uint64_t A = A0 + OB_LINE * tid;
      if (A >= len) break;
      const uint32_t nb = len - A < OB_LINE ? (uint32_t)(len - A) : OB_LINE;
      store_line(pack, off + A, low_bytes(load_bytes(out + A, nb), nb));
    }
  }
}

}  // namespace

extern "C" {

uint64_t xyws_outbox_scratch_bytes(uint64_t n) { return sizeof(ob_plan) * n + sizeof(ob_tile) * tiles_for(n); }

int xyws_outbox_map(void* pinned_host, void** dev_ptr) {
  if (!dev_ptr) return XYWS_ERR_INVALID;
  *dev_ptr = nullptr;
  if (!pinned_host) return XYWS_ERR_INVALID;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, pinned_host, 0) != hipSuccess || !d) {
    (void)hipGetLastError();  // (not mapped: the refusal is the answer, no error is left behind)
    return XYWS_ERR_INVALID;
  }
  *dev_ptr = d;
  return XYWS_OK;
}

int xyws_outbox_streams(xyws_ctx* ctx, const xyws_outbox_conn* dev_conns, uint64_t n, void* pack, uint64_t pack_cap,
                        xyws_outbox_entry* entries, xyws_outbox_summary* summary, void* dev_scratch,
                        uint64_t scratch_bytes, void* stream) {
  if (!ctx || (n && (!dev_conns || !entries || !summary || !dev_scratch))) return XYWS_ERR_INVALID;
  if (n >= UINT32_MAX || scratch_bytes < xyws_outbox_scratch_bytes(n)) return XYWS_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(pack) & 15u) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint64_t cap = pack ? pack_cap & ~15ull : 0, n_tiles = tiles_for(n);
  ob_plan* const plan = static_cast<ob_plan*>(dev_scratch);
  ob_tile* const tiles = reinterpret_cast<ob_tile*>(plan + n);
  hipLaunchKernelGGL(k_outbox_plan, dim3((uint32_t)n_tiles), dim3(OB_TILE), 0, (hipStream_t)stream, dev_conns, n, plan,
                     tiles);
  int rc = hip_err(hipGetLastError());
  if (rc != XYWS_OK) return rc;
  hipLaunchKernelGGL(k_outbox_scan, dim3(1), dim3(OB_SCAN_THREADS), 0, (hipStream_t)stream, plan, n, tiles, n_tiles, cap,
                     summary);
  rc = hip_err(hipGetLastError());
  if (rc != XYWS_OK) return rc;
  const dim3 grid = fanout_grid(n, cap != 0, OB_GRID_CAP, OB_BLOCKS_AIM, OB_SLICES_MAX);
  hipLaunchKernelGGL(k_outbox_pack, grid, dim3(OB_THREADS), 0, (hipStream_t)stream, dev_conns, n, plan, tiles,
                     pack, cap, entries);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of the three
// kernels. out: {connections per tile of the plan pass, bytes per step of the
// pack pass, its largest grid x, its largest grid y}.
int xyws_debug_outbox_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = OB_TILE;
  out[1] = OB_STEP;
  out[2] = OB_GRID_CAP;
  out[3] = OB_SLICES_MAX;
  return XYWS_OK;
}

// Internal (measurements): what a caller without xyws_outbox_streams does once
// it has the lengths on the host: one device-to-host copy per sender, issued
// one after another on `stream` by the calling thread, sender i's bytes to
// the offset its slot would have (scripts/outbox_rate.py). host_conns: a host
// copy of the conn table.
int xyws_debug_outbox_host_fetch(const xyws_outbox_conn* host_conns, const uint64_t* host_lens, uint64_t n,
                                 void* pinned_dst, uint64_t dst_cap, void* stream) {
  if (n && (!host_conns || !host_lens || !pinned_dst)) return XYWS_ERR_INVALID;
  uint64_t off = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t len = host_lens[i], slot = (len + 15u) & ~15ull;
    if (!len) continue;
    if (off + slot > dst_cap) return XYWS_ERR_CAPACITY;
    if (hipMemcpyAsync((uint8_t*)pinned_dst + off, host_conns[i].out, len, hipMemcpyDeviceToHost, (hipStream_t)stream) !=
        hipSuccess)
      return XYWS_ERR_HIP;
    off += slot;
  }
  return XYWS_OK;
}

}  // extern "C"
