// xyws_inbox.hip — xyws_inbox_streams: the received bytes of a whole sweep
// scattered from one dense pack into the connections' receive ranges, with the
// per-connection carry (HTTP, open or dead) and the buf and len words of the
// resident xyws_conn and xyws_accept_conn rows (the reference gives every
// socket a recv buffer of its own, include/xynet/stream_buffer/recv_all.h:86-121;
// here the completion queue's bytes arrive as one pack and an entry list). The
// semantics are stated in include/xyws.h; this is how they are computed. Every
// table row is read and written through xyws_rows.h, which names its words.
//
// Five launches, dev_scratch the hand-over between them. No workgroup waits
// for another inside a launch and nothing spins.
//
// k_inbox_clear: zeroes the globals and the per-connection accumulators.
//
// k_inbox_entries: one thread per entry, striding over m_cap. The only pass
// that reads the head and the entries (they may lie across the host link: an
// entry is loaded once, the head once per workgroup, since a workgroup that
// waited for another's M would be a dependency between workgroups): it
// keeps M and a record per entry in scratch, and adds each valid entry into
// its connection's accumulator with integer atomics (a sum, a maximum, a
// count and flag bits: the results do not depend on the order).
//
// k_inbox_conns: one thread per connection, one workgroup per tile of IB_TILE.
// The state step and the placement decision of a connection, its rows, carry
// and result row, the base its entries are placed at (or IB_NO_BASE), and the
// tile's sums by workgroup scans (block_scan, xyws_room.h).
//
// k_inbox_summary: one workgroup adds the tile sums and writes the summary.
//
// k_inbox_copy: blockIdx.x strides over the entries, blockIdx.y over
// IB_STEP-byte chunks of an entry (the host knows no M and no length: the grid
// comes from m_cap alone, as k_outbox_pack's comes from n). A chunk is one
// wave's copy_span (xyws_lines.h): whole lines by 16-byte stores, the first and
// last line of an entry's destination byte by byte, so nothing outside
// [buf + A + at, buf + A + at + len) is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_lines.h"
#include "xyws_room.h"
#include "xyws_rows.h"

#define IB_WAVE BC_WAVE
#define IB_TILE 256u            // connections per workgroup of the connection pass, entries per workgroup of the entry pass
#define IB_THREADS 64u          // the copy pass: one wave per workgroup
#define IB_LINE 16u             // bytes a thread writes per copy step
#define IB_STEP (IB_LINE * IB_THREADS)  // bytes a workgroup writes per step
#define IB_ENTRY_GRID_CAP 256u  // workgroups of the clear and entry passes (one per CU); further items are grid-strided
#define IB_GRID_CAP 4096u       // entries per launch of the copy pass in x; further ones are grid-strided
#define IB_BLOCKS_AIM 16384u    // one-wave workgroups wanted in flight (256 CUs x 64)
#define IB_SLICES_MAX 64u       // at most this many workgroups share one entry

static_assert(IB_TILE % IB_WAVE == 0 && IB_TILE >= 16, "whole waves; the summary pass stores one word per thread");

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

// dev_scratch: the globals, n accumulators, m_cap entry records, the tile sums.
struct ib_globals { uint64_t m, n_bad, clipped, reserved[5]; };
// A connection's accumulator: the entry pass adds into t, s and meta; the
// connection pass leaves in `base` where the copy pass places its entries.
struct ib_acc {
  uint64_t t;     // max(at + len) over its valid entries
  uint64_t s;     // sum of len over them
  uint64_t meta;  // entries that named it | IB_F_* << 32
  uint64_t base;  // A, or IB_NO_BASE: nothing of it is placed
};
// An entry as the copy pass needs it. tag: conn, and IB_E_COPY when it is valid and has bytes.
struct ib_ent { uint64_t tag, off, len, at; };
struct ib_tile { uint64_t bytes, counts; };  // counts: n_conns | n_opened << 16 | n_eof << 32 | n_broken << 48
constexpr uint64_t IB_F_EOF = 1ull << 32, IB_F_BAD_RANGE = 1ull << 33;
constexpr uint64_t IB_E_COPY = 1ull << 32;
constexpr uint64_t IB_NO_BASE = ~0ull;
typedef unsigned long long ull;
// (scratch is device memory: global loads and stores, the records by their fields)
typedef XYWS_GLOBAL ib_globals g_globals;
typedef XYWS_GLOBAL ib_acc g_acc;
typedef XYWS_GLOBAL ib_ent g_ent;
typedef XYWS_GLOBAL ib_tile g_tile;

__host__ __device__ inline uint64_t tiles_for(uint64_t n) { return (n + IB_TILE - 1u) / IB_TILE; }

struct ib_scratch {
  ib_globals* globals;
  ib_acc* acc;
  ib_ent* ent;
  ib_tile* tiles;
};
inline ib_scratch carve(void* mem, uint64_t n, uint64_t m_cap) {
  ib_scratch s;
  s.globals = static_cast<ib_globals*>(mem);
  s.acc = reinterpret_cast<ib_acc*>(s.globals + 1);
  s.ent = reinterpret_cast<ib_ent*>(s.acc + n);
  s.tiles = reinterpret_cast<ib_tile*>(s.ent + m_cap);
  return s;
}

__global__ void __launch_bounds__(IB_TILE) k_inbox_clear(uint64_t* words, uint64_t n_words) {
  XYWS_GLOBAL uint64_t* const w = (XYWS_GLOBAL uint64_t*)words;
  for (uint64_t k = (uint64_t)blockIdx.x * IB_TILE + threadIdx.x; k < n_words; k += (uint64_t)gridDim.x * IB_TILE) w[k] = 0;
}

__global__ void __launch_bounds__(IB_TILE)
    k_inbox_entries(const xyws_inbox_head* __restrict__ head, const xyws_inbox_entry* __restrict__ entries, uint64_t m_cap,
                    uint64_t n, uint64_t pack_cap, ib_globals* globals, ib_acc* acc, ib_ent* ent) {
  __shared__ uint64_t s_head[2];
  const uint32_t tid = threadIdx.x;
  g_globals* const g = (g_globals*)globals;
  if (tid == 0) {
    const rows::inbox_head_row h = rows::load_inbox_head(head);
    s_head[0] = h.m < m_cap ? h.m : m_cap;
    s_head[1] = h.pack_len < pack_cap ? h.pack_len : pack_cap;
    if (blockIdx.x == 0) {
      g->m = s_head[0];
      g->clipped = h.m > m_cap ? 1u : 0u;
    }
  }
  __syncthreads();
  const uint64_t M = uniform64(s_head[0]), P = uniform64(s_head[1]);
  for (uint64_t k = (uint64_t)blockIdx.x * IB_TILE + tid; k < M; k += (uint64_t)gridDim.x * IB_TILE) {
    const rows::inbox_entry_row e = rows::load_inbox_entry(entries + k);
    uint64_t tag = e.tag.conn;
    if (e.tag.conn >= n) {  // rule 1: ignored and counted
      atomicAdd((ull*)&globals->n_bad, 1ull);
    } else {
      ib_acc* const a = acc + e.tag.conn;
      const bool in_pack = e.off <= P && e.len <= P - e.off;
      uint64_t add = 1ull | (e.tag.flags & XYWS_IBE_EOF ? IB_F_EOF : 0ull);
      if (in_pack) {
        atomicAdd((ull*)&a->s, (ull)e.len);
        atomicMax((ull*)&a->t, (ull)sat_add(e.at, e.len));
        if (e.len) tag |= IB_E_COPY;
      } else {
        atomicAdd((ull*)&globals->n_bad, 1ull);
        add |= IB_F_BAD_RANGE;
      }
      // (the count is below 2^32, so adding 1 never carries into the flag bits; the flags are or-ed)
      atomicAdd((ull*)&a->meta, 1ull);
      if (add >> 32) atomicOr((ull*)&a->meta, (ull)(add & ~0xFFFFFFFFull));
    }
    g_ent* const r = (g_ent*)(ent + k);
    r->tag = tag;
    r->off = e.off;
    r->len = e.len;
    r->at = e.at;
  }
}

__global__ void __launch_bounds__(IB_TILE)
    k_inbox_conns(const xyws_inbox_conn* __restrict__ iconns, uint64_t n, ib_acc* acc, ib_tile* __restrict__ tiles,
                  xyws_inbox_result* __restrict__ results) {
  __shared__ uint64_t s_w[IB_TILE / IB_WAVE];
  const uint32_t tid = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * IB_TILE + tid;
  uint64_t placed = 0, counts = 0;
  if (i < n) {
    const rows::inbox_conn_row ic = rows::load_inbox_conn(iconns + i);
    rows::inbox_carry_row cr = rows::load_inbox_carry((const xyws_inbox_carry*)ic.carry);
    g_acc* const a = (g_acc*)(acc + i);
    const uint64_t T = a->t, S = a->s, meta = a->meta;
    const uint32_t cnt = (uint32_t)meta;
    uint32_t st = cr.state.state, sticky = cr.state.status, now = 0;
    uint64_t A = 0, kept = 0, lead = 0;
    bool opened = false, broken = false;
    if (meta & IB_F_EOF) sticky |= XYWS_IBR_EOF;  // rule 6
    // rule 3
    if (st >= XYWS_IB_DEAD) {
      st = XYWS_IB_DEAD;
    } else if (st == XYWS_IB_HTTP) {
      if (ic.flags & XYWS_IBC_NO_HANDSHAKE) {
        st = XYWS_IB_OPEN;
        cr.http_len = 0;
      } else if (ic.aresult) {
        const rows::accept_end v = rows::load_accept_end((const xyws_accept_result*)ic.aresult);
        if (v.status & XYWS_ACC_REJECTED) {
          st = XYWS_IB_DEAD;
          sticky |= XYWS_IBR_REFUSED;
        } else if (v.status & XYWS_ACC_ACCEPTED) {
          if (v.consumed > cr.http_len) {
            broken = true;
            sticky |= XYWS_IBR_BAD_CONSUMED;
          } else {
            opened = true;
            st = XYWS_IB_OPEN;
            kept = cr.http_len - v.consumed;
            lead = kept ? v.consumed : 0;
          }
        }
      }
    }
    if (st == XYWS_IB_DEAD) {
      if (cnt) now |= XYWS_IBR_DROPPED;
    } else {
      // rule 4
      if (!broken) A = (st == XYWS_IB_HTTP || kept) ? cr.http_len : 0;
      if (meta & IB_F_BAD_RANGE) sticky |= XYWS_IBR_BAD_RANGE, broken = true;
      if (S != T) sticky |= XYWS_IBR_BAD_TILING, broken = true;
      if (T > ic.cap || A > ic.cap - T) sticky |= XYWS_IBR_OVERFLOW, broken = true;
      if (broken) {
        st = XYWS_IB_DEAD;
        opened = false;
        kept = lead = 0;
      } else {
        placed = T;
      }
    }
    // rule 5
    uint64_t conn_buf = ic.buf, conn_len = 0, acc_len = 0;
    if (st == XYWS_IB_OPEN) {
      conn_buf = ic.buf + lead;
      conn_len = kept + T;
      cr.http_len = 0;
    } else if (st == XYWS_IB_HTTP) {
      cr.http_len += T;
      acc_len = T ? cr.http_len : 0;
    }
    if (ic.conn) rows::store_conn_recv((xyws_conn*)ic.conn, conn_buf, conn_len);
    if (ic.aconn) rows::store_accept_recv((xyws_accept_conn*)ic.aconn, ic.buf, acc_len);
    cr.bytes_total += placed;
    cr.state = {st, sticky};
    rows::store_inbox_carry((xyws_inbox_carry*)ic.carry, cr);
    if (results)
      rows::store_inbox_result(results + i, placed, lead, {cnt, sticky | now | (opened ? XYWS_IBR_OPENED : 0u)});
    a->base = placed ? A : IB_NO_BASE;
    counts = (cnt ? 1ull : 0ull) | (opened ? 1ull << 16 : 0ull) | (meta & IB_F_EOF ? 1ull << 32 : 0ull) |
             (broken ? 1ull << 48 : 0ull);
  }
  uint64_t t_bytes, t_counts;
  block_scan<IB_TILE / IB_WAVE>(placed, tid, s_w, t_bytes);
  block_scan<IB_TILE / IB_WAVE>(counts, tid, s_w, t_counts);
  if (tid == 0) {
    g_tile* const t = (g_tile*)(tiles + blockIdx.x);
    t->bytes = t_bytes;
    t->counts = t_counts;
  }
}

__global__ void __launch_bounds__(IB_TILE)
    k_inbox_summary(const ib_globals* __restrict__ globals, const ib_tile* __restrict__ tiles, uint64_t n_tiles,
                    xyws_inbox_summary* __restrict__ summary) {
  __shared__ uint64_t s_w[IB_TILE / IB_WAVE];
  const uint32_t tid = threadIdx.x;
  uint64_t a_bytes = 0, a_conns = 0, a_opened = 0, a_eof = 0, a_broken = 0;
  for (uint64_t t = tid; t < n_tiles; t += IB_TILE) {
    const g_tile* const w = (const g_tile*)(tiles + t);
    const uint64_t c = w->counts;
    a_bytes += w->bytes;
    a_conns += c & 0xFFFFu;
    a_opened += (c >> 16) & 0xFFFFu;
    a_eof += (c >> 32) & 0xFFFFu;
    a_broken += c >> 48;
  }
  uint64_t bytes, conns, opened, eof, broken;
  block_scan<IB_TILE / IB_WAVE>(a_bytes, tid, s_w, bytes);
  block_scan<IB_TILE / IB_WAVE>(a_conns, tid, s_w, conns);
  block_scan<IB_TILE / IB_WAVE>(a_opened, tid, s_w, opened);
  block_scan<IB_TILE / IB_WAVE>(a_eof, tid, s_w, eof);
  block_scan<IB_TILE / IB_WAVE>(a_broken, tid, s_w, broken);
  if (tid < rows::IBS_WORDS) {
    const g_globals* const g = (const g_globals*)globals;
    const uint64_t n_bad = g->n_bad;
    uint64_t w[rows::IBS_WORDS];
    rows::pack_inbox_summary({g->m, bytes, {(uint32_t)conns, (uint32_t)opened}, {(uint32_t)eof, (uint32_t)broken},
                              {(uint32_t)n_bad, (n_bad ? XYWS_IBM_BAD_ENTRIES : 0u) | (broken ? XYWS_IBM_BROKEN : 0u) |
                                                    (g->clipped ? XYWS_IBM_CLIPPED : 0u)}},
                             w);
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < rows::IBS_WORDS; k++) mine = tid == k ? w[k] : mine;
    rows::store_inbox_summary_word(summary, tid, mine);
  }
}

__global__ void __launch_bounds__(IB_THREADS)
    k_inbox_copy(const xyws_inbox_conn* __restrict__ iconns, const ib_globals* __restrict__ globals,
                 const ib_acc* __restrict__ acc, const ib_ent* __restrict__ ent, const void* pack_mem) {
  const uint32_t tid = threadIdx.x;
  const uint64_t M = uniform64(((const g_globals*)globals)->m);  // (at most m_cap: the records behind it were never written)
  const uint64_t pack = (uint64_t)(uintptr_t)pack_mem;
  for (uint64_t k = blockIdx.x; k < M; k += gridDim.x) {
    const g_ent* const e = (const g_ent*)(ent + k);
    const uint64_t tag = uniform64(e->tag);
    if (!(tag & IB_E_COPY)) continue;
    const uint64_t ci = tag & 0xFFFFFFFFull;  // (below n: the entry pass checked it)
    const uint64_t A = uniform64(((const g_acc*)(acc + ci))->base);
    if (A == IB_NO_BASE) continue;
    // the connection pass found A + T <= cap and at + len <= T: the destination lies inside the range
    const uint64_t d = rows::load_inbox_buf(iconns + ci) + A + uniform64(e->at), len = uniform64(e->len);
    const uint64_t P0 = d & 15u;
    copy_span((g_u8*)(d & ~15ull), P0, P0 + len, pack + uniform64(e->off), (uint64_t)blockIdx.y * IB_STEP,
              (uint64_t)gridDim.y * IB_STEP, tid);
  }
}

}  // namespace

extern "C" {

uint64_t xyws_inbox_scratch_bytes(uint64_t n, uint64_t m_cap) {
  return sizeof(ib_globals) + sizeof(ib_acc) * n + sizeof(ib_ent) * m_cap + sizeof(ib_tile) * tiles_for(n);
}

int xyws_inbox_streams(xyws_ctx* ctx, const xyws_inbox_conn* dev_iconns, uint64_t n, const xyws_inbox_head* head,
                       const xyws_inbox_entry* entries, uint64_t m_cap, const void* pack, uint64_t pack_cap,
                       xyws_inbox_result* dev_results, xyws_inbox_summary* summary, void* dev_scratch,
                       uint64_t scratch_bytes, void* stream) {
  if (!ctx || (n && (!dev_iconns || !head || !summary || !dev_scratch))) return XYWS_ERR_INVALID;
  if ((m_cap && !entries) || (pack_cap && !pack)) return XYWS_ERR_INVALID;
  if (n >= UINT32_MAX || m_cap >= UINT32_MAX) return XYWS_ERR_INVALID;
  if (n && ((reinterpret_cast<uintptr_t>(dev_scratch) & 7u) || scratch_bytes < xyws_inbox_scratch_bytes(n, m_cap)))
    return XYWS_ERR_INVALID;  // (the accumulators take 64-bit atomics)
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  hipStream_t const q = (hipStream_t)stream;
  const ib_scratch s = carve(dev_scratch, n, m_cap);
  const uint64_t n_tiles = tiles_for(n), clear_words = (sizeof(ib_globals) + sizeof(ib_acc) * n) / 8;
  hipLaunchKernelGGL(k_inbox_clear, dim3(grid_for(clear_words, IB_TILE, IB_ENTRY_GRID_CAP)), dim3(IB_TILE), 0, q,
                     reinterpret_cast<uint64_t*>(dev_scratch), clear_words);
  int rc = hip_err(hipGetLastError());
  if (rc != XYWS_OK) return rc;
  hipLaunchKernelGGL(k_inbox_entries, dim3(grid_for(m_cap, IB_TILE, IB_ENTRY_GRID_CAP)), dim3(IB_TILE), 0, q, head, entries,
                     m_cap, n, pack_cap, s.globals, s.acc, s.ent);
  rc = hip_err(hipGetLastError());
  if (rc != XYWS_OK) return rc;
  hipLaunchKernelGGL(k_inbox_conns, dim3((uint32_t)n_tiles), dim3(IB_TILE), 0, q, dev_iconns, n, s.acc, s.tiles, dev_results);
  rc = hip_err(hipGetLastError());
  if (rc != XYWS_OK) return rc;
  hipLaunchKernelGGL(k_inbox_summary, dim3(1), dim3(IB_TILE), 0, q, s.globals, s.tiles, n_tiles, summary);
  rc = hip_err(hipGetLastError());
  if (rc != XYWS_OK) return rc;
  const dim3 grid = fanout_grid(m_cap, m_cap != 0 && pack_cap != 0, IB_GRID_CAP, IB_BLOCKS_AIM, IB_SLICES_MAX);
  hipLaunchKernelGGL(k_inbox_copy, grid, dim3(IB_THREADS), 0, q, dev_iconns, s.globals, s.acc, s.ent, pack);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of the kernels.
// out: {connections per tile of the connection pass (and entries per workgroup
// of the entry pass), bytes per step of the copy pass, its largest grid x, its
// largest grid y, the largest grid of the entry pass}.
int xyws_debug_inbox_geometry(uint64_t out[5]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = IB_TILE;
  out[1] = IB_STEP;
  out[2] = IB_GRID_CAP;
  out[3] = IB_SLICES_MAX;
  out[4] = IB_ENTRY_GRID_CAP;
  return XYWS_OK;
}

// Internal (measurements): what a caller without xyws_inbox_streams does with
// the bytes of a sweep: one host-to-device copy per receiving connection, issued
// one after another on `stream` by the calling thread (scripts/inbox_rate.py).
// Entry k: lens[k] bytes from pinned_src + src_offs[k] to the device address dsts[k].
int xyws_debug_inbox_host_scatter(const uint64_t* dsts, const uint64_t* src_offs, const uint64_t* lens, uint64_t m,
                                  const void* pinned_src, void* stream) {
  if (m && (!dsts || !src_offs || !lens || !pinned_src)) return XYWS_ERR_INVALID;
  for (uint64_t k = 0; k < m; k++) {
    if (!lens[k]) continue;
    if (hipMemcpyAsync((void*)(uintptr_t)dsts[k], (const uint8_t*)pinned_src + src_offs[k], lens[k], hipMemcpyHostToDevice,
                       (hipStream_t)stream) != hipSuccess)
      return XYWS_ERR_HIP;
  }
  return XYWS_OK;
}

}  // extern "C"
