// xyws_accept.hip — xyws_accept_streams: the opening handshakes of many
// connections answered by one launch (the reference's websocket_request_handler
// as websocket_handshake drives it, example/include/common/websocket.h:40-68,
// run once per coroutine). The semantics are stated in include/xyws.h, the
// grammar, the checks, SHA-1 and base64 in xyws_accept.h; this is how the
// device runs them.
//
// As in k_reply_streams connections are independent: one wave (a 64-thread
// workgroup) takes one connection, connections are grid-strided, no workgroup
// talks to another and nothing spins. Per connection:
//   1. stage: the lanes load the whole aligned 16-byte lines that hold
//      buf[0, E), E = min(len, max_request), into LDS at the same line
//      offsets, one line per lane per step (with max_request 1024 one step);
//   2. walk: the wave runs xyws_accept.h's evaluate() over the staged bytes:
//      the grammar is defined by its sequential walk, and this is that walk,
//      the same source xyws_accept_request compiles for the host, taken by
//      all lanes together on scalar registers (staged_bytes below). SHA-1 and
//      base64 are wave-uniform too. The verdict stays in registers, the whole
//      response (at most 129 bytes) goes to LDS;
//   3. send: the lanes write the response to the send range in 16-byte lines
//      (xyws_lines.h), one line per lane; lane 0 writes the result row.
// LDS is sized by the launch: the staged lines of max_request bytes at any
// alignment and the response.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_lines.h"
#include "xyws_accept.h"
#include "xyws_rows.h"

#define ACCEPT_LANES 64u       // lanes per connection: one wave
#define ACCEPT_LINE 16u        // bytes a lane stages or writes per step
#define ACCEPT_GRID_CAP 8192u  // 256 CUs x 32 one-wave workgroups; further connections are grid-strided

typedef __attribute__((address_space(3))) uint64_t l_u64;

using namespace xyws_internal;

// The staged lines of a request of up to max_request bytes at any alignment.
__host__ __device__ inline uint32_t stage_bytes(uint32_t max_request) { return ((max_request + 30u) >> 4) << 4; }
__host__ __device__ inline uint32_t lds_bytes(uint32_t max_request) {
  return stage_bytes(max_request) + xyws_accept::RESP_MAX;
}

// Request byte i is staged byte lo + i. The whole wave walks together: every
// lane reads the same 8 staged bytes (one LDS read per 8 bytes of a forward
// walk) and the word goes to scalar registers, so the byte, the position and
// every decision of the walk are wave-uniform: scalar compares and branches,
// no divergence, and the verdict needs no hand-over. It is no faster than one
// lane walking alone (measured both ways): a wave takes about
// 70 us for a 499-byte request either way, the walk being one dependent chain.
struct staged_bytes {
  const l_u64* w;  // the staged lines as 8-byte words
  uint32_t lo;
  mutable uint32_t at = 0xFFFFFFFFu;  // index of the word held
  mutable uint64_t held = 0;
  XYWS_DEV uint8_t operator[](uint32_t i) const {
    const uint32_t q = lo + i, wi = q >> 3;
    if (wi != at) {
      at = wi;
      held = uniform64(w[wi]);
    }
    return (uint8_t)(held >> (8u * (q & 7u)));
  }
};

__global__ void __launch_bounds__(ACCEPT_LANES) k_accept_streams(const xyws_accept_conn* __restrict__ conns, uint64_t n,
                                                                 uint32_t max_request, uint32_t policy,
                                                                 xyws_accept_result* __restrict__ results) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
  uint8_t* const s_resp = s_mem + stage_bytes(max_request);
  const uint32_t lane = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const xyws_rows::accept_conn_row cq = xyws_rows::load_accept_conn(conns + ci);
    const uint64_t buf = cq.buf, len = cq.len, out = cq.out, out_cap = cq.out_cap;
    const uint32_t E = len < max_request ? (uint32_t)len : max_request;
    const uint32_t lo = (uint32_t)(buf & 15u);

    // 1. the lines that hold buf[0, E): at most stage_bytes / 16
    const g_u8* const base = (const g_u8*)(buf & ~15ull);
    const uint32_t nlines = E ? (lo + E + 15u) >> 4 : 0u;
    for (uint32_t li = lane; li < nlines; li += ACCEPT_LANES)
      *reinterpret_cast<u32x4*>(s_mem + ACCEPT_LINE * li) = *reinterpret_cast<const g_u32x4*>(base + ACCEPT_LINE * li);
    __syncthreads();

    // 2. the sequential walk, by the whole wave (every lane writes the same response bytes)
    const xyws_accept::verdict v =
        xyws_accept::evaluate(staged_bytes{(const l_u64*)s_mem, lo}, E, len >= max_request, policy, s_resp);
    __syncthreads();

    // 3. response byte q at position olo + q from obase
    const uint32_t resp_len = v.resp_len;
    g_u8* const obase = (g_u8*)(out & ~15ull);
    const uint64_t olo = out & 15u;
    const uint64_t wlim = sat_add(olo, out_cap), P1 = olo + resp_len;
    const uint64_t wl = P1 < wlim ? P1 : wlim;
    const uint64_t A = (uint64_t)ACCEPT_LINE * lane;  // (129 + 15 bytes: one step)
    if (wl > olo && A < wl) {
      const uint64_t s = A > olo ? A : olo, e = A + 16 < P1 ? A + 16 : P1;
      bytes16 acc = {0, 0};
      for (uint32_t a = (uint32_t)(s - A), ae = (uint32_t)(e - A); a < ae; a++) {
        const uint64_t c = s_resp[(uint32_t)(A + a - olo)];
        if (a < 8) acc.lo |= c << (8u * a);
        else acc.hi |= c << (8u * (a - 8));
      }
      put_line(obase, A, s, e, olo, wlim, acc);
    }
    if (lane == 0 && results) {
      const uint32_t st = v.status | (resp_len > out_cap ? XYWS_ACC_TRUNCATED : 0u);
      xyws_rows::store_accept_result(results + ci, {st, v.http_status, v.reason, v.consumed, resp_len, v.path_off,
                                                    v.path_len, v.key_off});
    }
    __syncthreads();  // (LDS is rewritten by the next connection)
  }
}

extern "C" {

int xyws_accept_streams(xyws_ctx* ctx, const xyws_accept_conn* dev_conns, uint64_t n, uint32_t max_request,
                        uint32_t policy, xyws_accept_result* dev_results, void* stream) {
  if (!ctx || (n && !dev_conns)) return XYWS_ERR_INVALID;
  if (!xyws_accept::args_ok(max_request, policy)) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, ACCEPT_GRID_CAP);
  hipLaunchKernelGGL(k_accept_streams, dim3(grid), dim3(ACCEPT_LANES), lds_bytes(max_request), (hipStream_t)stream,
                     dev_conns, n, max_request, policy, dev_results);
  return hip_err(hipGetLastError());
}

int xyws_accept_request(const void* host_req, uint64_t len, uint32_t max_request, uint32_t policy, void* host_out,
                        uint64_t out_cap, xyws_accept_result* res) {
  return xyws_accept::accept_request(host_req, len, max_request, policy, host_out, out_cap, res);
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_accept_streams. out: {lanes per connection, LDS bytes per wave at
// XYWS_ACCEPT_MAX_REQUEST, lines staged per step, grid cap}.
int xyws_debug_accept_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = ACCEPT_LANES;
  out[1] = lds_bytes(XYWS_ACCEPT_MAX_REQUEST);
  out[2] = ACCEPT_LANES;
  out[3] = ACCEPT_GRID_CAP;
  return XYWS_OK;
}

// Internal (measurements, no HIP call): xyws_accept_request over n requests of
// len bytes each in one host slab, on the calling thread: what a caller without
// xyws_accept_streams runs between its two copies (scripts/accept_rate.py).
int xyws_debug_accept_host(const void* host_reqs, uint64_t req_stride, uint64_t len, uint64_t n, uint32_t max_request,
                           uint32_t policy, void* host_outs, uint64_t out_stride, uint64_t out_cap,
                           xyws_accept_result* host_results) {
  if (n && (!host_reqs || !host_results || (out_cap && !host_outs))) return XYWS_ERR_INVALID;
  for (uint64_t i = 0; i < n; i++) {
    const int rc = xyws_accept::accept_request((const uint8_t*)host_reqs + req_stride * i, len, max_request, policy,
                                               out_cap ? (uint8_t*)host_outs + out_stride * i : nullptr, out_cap,
                                               host_results + i);
    if (rc) return rc;
  }
  return XYWS_OK;
}

}  // extern "C"
