// xyws_unsent.hip — xyws_unsent_streams and xyws_unsent_view_streams: the send
// bytes a socket did not take stay on the device, right-aligned in front of the
// connection's send range (the reference keeps m_write_msgs per session and
// drains it as the socket allows, example/websocket/websocket_chat.cpp:148-175).
// The semantics are stated in include/xyws.h; this is how they are computed.
// Every table row is read and written through xyws_rows.h, which names its words.
//
// k_unsent, one launch: a workgroup of four waves per tile of US_TILE
// connections. No workgroup waits for another, nothing spins, no atomics.
//  - plan: one thread per connection loads its row, its carry and its report,
//    decides the tail and writes the carry and the result row. A sweep in which
//    every socket took everything ends here: three row reads per connection and
//    no payload byte.
//  - scan: the connections whose tail has to move are compacted by a workgroup
//    scan (block_scan, xyws_room.h); their move records go to the tile's part
//    of dev_scratch.
//  - move: the tile's waves take the records in turn, a wave per connection.
//    The tail is an overlapping memmove between two ranges of different 16-byte
//    phase. The wave walks the destination's lines, 64 lines of 16 bytes per
//    step, ascending when the destination lies below the source and descending
//    when above; a lane composes its line from one or two aligned source lines
//    (load_bytes: the funnel of xyws_lines.h) and ends it with put_line: a whole
//    store inside the tail, byte stores of its own bytes on the two edge lines,
//    which neighbours share. Every load of a step is issued, and waited for by
//    the whole wave, before the step's first store; the steps before it wrote
//    only destination bytes on the far side of everything it reads. A tail is
//    never split over waves: a second wave on the same tail could store over a
//    line the first has yet to load, and nothing orders two waves without a
//    wait.
//
// k_unsent_view, one launch, one thread per connection: the view row, the
// synthesized backlog row and the carry's last_len. No payload byte is touched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_lines.h"
#include "xyws_outbox.h"
#include "xyws_room.h"
#include "xyws_rows.h"

#define US_WAVE BC_WAVE
#define US_TILE 256u                    // connections per workgroup: one per thread of the plan, four waves
#define US_WAVES (US_TILE / US_WAVE)    // the waves that share a tile's moves
#define US_LINE 16u                     // bytes a lane moves per step
#define US_STEP (US_LINE * US_WAVE)     // bytes a wave moves per step

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

// dev_scratch: a move record per connection; tile b's k-th record is record
// US_TILE * b + k. up: the destination lies below the source (ascending steps).
struct us_move { uint64_t src, dst, len, up; };
typedef XYWS_GLOBAL us_move g_move;

__host__ __device__ inline uint64_t tiles_for(uint64_t n) { return (n + US_TILE - 1u) / US_TILE; }

// The t bytes at src to dst, by one wave (src != dst, t > 0; the ranges may overlap).
XYWS_DEV void move_tail(uint64_t src, uint64_t dst, uint64_t t, bool up, uint32_t lane) {
  g_u8* const base = (g_u8*)(dst & ~15ull);
  const uint64_t P0 = dst & 15u, P1 = P0 + t, steps = (P1 + US_STEP - 1u) / US_STEP;
  for (uint64_t k = 0; k < steps; k++) {
    const uint64_t A = (up ? k : steps - 1u - k) * US_STEP + US_LINE * lane;
    const bool mine = A < P1;
    const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
    bytes16 v = {0, 0};
    if (mine) {
      const uint32_t nb = (uint32_t)(e - s);
      v = shl_bytes(low_bytes(load_bytes(src + (s - P0), nb), nb), (uint32_t)(s - A));
    }
    // every lane's lines are in registers before any lane stores
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (mine) put_line(base, A, s, e, P0, P1, v);
  }
}

__global__ void __launch_bounds__(US_TILE)
    k_unsent(const xyws_unsent_conn* __restrict__ uconns, uint64_t n, const xyws_unsent_report* __restrict__ reports,
             const xyws_unsent_head* __restrict__ head, xyws_unsent_result* __restrict__ results, us_move* __restrict__ list) {
  __shared__ uint64_t s_w[US_WAVES];
  const uint32_t tid = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * US_TILE + tid;
  us_move m = {0, 0, 0, 0};
  uint64_t listed = 0;
  __shared__ uint32_t s_sweep;  // (the head may lie in pinned memory: it crosses the host link once per workgroup)
  if (tid == 0) s_sweep = rows::load_unsent_sweep(head);
  __syncthreads();
  if (i < n) {
    const rows::unsent_conn_row c = rows::load_unsent_conn(uconns + i);
    uint64_t pend = 0;
    uint32_t status = 0;
    if (c.carry) {
      xyws_unsent_carry* const carry = (xyws_unsent_carry*)c.carry;
      const rows::unsent_carry_row old = rows::load_unsent_carry(carry);
      const uint32_t sweep = s_sweep;
      uint64_t sent = old.last_len;  // no report of this sweep: the socket took everything
      if (reports) {
        const rows::unsent_report r = rows::load_unsent_report(reports + i);
        if (r.sweep == sweep) sent = r.sent;
      }
      if (sent > old.last_len) {
        sent = old.last_len;
        status |= XYWS_US_BAD_REPORT;
      }
      const uint64_t t = old.last_len - sent;
      if (t && c.out && t <= c.pend_cap) {
        // (a carry that says more than pend_cap was not left by this call: the range below `out` ends there)
        const uint64_t before = old.pend_len < c.pend_cap ? old.pend_len : c.pend_cap;
        pend = t;
        status |= XYWS_US_KEPT;
        m.src = c.out - before + sent;
        m.dst = c.out - t;
        if (m.src != m.dst) {
          m.len = t;
          m.up = m.dst < m.src;
          listed = 1;
        }
      } else if (t) {
        status |= XYWS_US_OVERFLOW;
      }
      rows::store_unsent_carry(carry, pend, pend, {sweep, status});
    }
    if (results) rows::store_unsent_result(results + i, pend, m.len, status);
  }
  uint64_t count;
  const uint64_t incl = block_scan<US_WAVES>(listed, tid, s_w, count);
  g_move* const mine = (g_move*)(list + (uint64_t)blockIdx.x * US_TILE);
  if (listed) {
    g_move* const r = mine + (incl - 1u);
    r->src = m.src;
    r->dst = m.dst;
    r->len = m.len;
    r->up = m.up;
  }
  __syncthreads();  // (the tile's records are written)
  const uint32_t lane = tid & (US_WAVE - 1u);
  for (uint64_t k = tid / US_WAVE; k < count; k += US_WAVES) {
    const g_move* const r = mine + k;
    move_tail(uniform64(r->src), uniform64(r->dst), uniform64(r->len), uniform64(r->up) != 0, lane);
  }
}

__global__ void __launch_bounds__(US_TILE)
    k_unsent_view(const xyws_unsent_conn* __restrict__ uconns, const xyws_outbox_conn* __restrict__ conns, uint64_t n,
                  xyws_outbox_conn* __restrict__ view, xyws_backlog_result* __restrict__ view_rows) {
  const uint64_t i = (uint64_t)blockIdx.x * US_TILE + threadIdx.x;
  if (i >= n) return;
  rows::outbox_conn_row c = rows::load_outbox_conn<false>(conns + i);
  const outbox_lengths r = outbox_rules(c);  // rule 1 of xyws_outbox_streams, over the caller's row
  xyws_unsent_carry* const carry = (xyws_unsent_carry*)rows::load_unsent_conn(uconns + i).carry;
  const uint64_t pend = carry && c.out ? rows::load_unsent_pend_len(carry) : 0;
  if (carry) rows::store_unsent_last_len(carry, pend + r.len);
  rows::store_backlog_send_len(view_rows + i, pend + r.full);
  if (c.out) {
    c.out -= pend;
    c.out_cap += pend;
  }
  c.backlog = (uint64_t)(uintptr_t)(view_rows + i);
  rows::store_outbox_conn(view + i, c);
}

}  // namespace

extern "C" {

uint64_t xyws_unsent_scratch_bytes(uint64_t n) { return sizeof(us_move) * n; }

int xyws_unsent_streams(xyws_ctx* ctx, const xyws_unsent_conn* dev_uconns, uint64_t n, const xyws_unsent_report* reports,
                        const xyws_unsent_head* head, xyws_unsent_result* dev_results, void* dev_scratch,
                        uint64_t scratch_bytes, void* stream) {
  if (!ctx || (n && (!dev_uconns || !head || !dev_scratch))) return XYWS_ERR_INVALID;
  if (n >= UINT32_MAX || scratch_bytes < xyws_unsent_scratch_bytes(n)) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  hipLaunchKernelGGL(k_unsent, dim3((uint32_t)tiles_for(n)), dim3(US_TILE), 0, (hipStream_t)stream, dev_uconns, n, reports,
                     head, dev_results, static_cast<us_move*>(dev_scratch));
  return hip_err(hipGetLastError());
}

int xyws_unsent_view_streams(xyws_ctx* ctx, const xyws_unsent_conn* dev_uconns, const xyws_outbox_conn* dev_conns, uint64_t n,
                             xyws_outbox_conn* dev_view, xyws_backlog_result* dev_view_rows, void* stream) {
  if (!ctx || (n && (!dev_uconns || !dev_conns || !dev_view || !dev_view_rows))) return XYWS_ERR_INVALID;
  if (n >= UINT32_MAX) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  hipLaunchKernelGGL(k_unsent_view, dim3((uint32_t)tiles_for(n)), dim3(US_TILE), 0, (hipStream_t)stream, dev_uconns,
                     dev_conns, n, dev_view, dev_view_rows);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of k_unsent.
// out: {connections per tile, bytes a wave moves per step, waves per tile,
// bytes of a move record in dev_scratch}.
int xyws_debug_unsent_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = US_TILE;
  out[1] = US_STEP;
  out[2] = US_WAVES;
  out[3] = sizeof(us_move);
  return XYWS_OK;
}

}  // extern "C"
