// xyws_route.hip — xyws_route_streams: the request targets of many accepted
// handshakes looked up in a device-resident route table by one launch, each
// connection's room stored into its roster row (the reference looks at
// websocket_request_handler::get_path on the host, one coroutine at a time).
// The semantics are stated in include/xyws.h, the table, the hash, the key of
// a target and its candidates in xyws_route.h; this is how the device runs
// them.
//
// As in k_accept_streams connections are independent: one wave (a 64-thread
// workgroup) takes one connection, connections are grid-strided, no workgroup
// talks to another and nothing spins. Per accepted connection:
//   1. stage: the lanes load the at most 17 aligned 16-byte lines that hold the
//      first min(path_len, 257) bytes of the target into LDS;
//   2. key: lane l takes target bytes 4l .. 4l + 3; a ballot finds the first
//      `?` or `#`, which with the trailing `/` gives the key's length;
//   3. hash: each lane hashes its four bytes, one wave scan (six shuffle
//      steps; the polynomial hash of two halves composes, xyws_route.h) gives
//      every lane the hash of the target up to its first byte, and four more
//      steps per lane the hash of every prefix of the key's window;
//   4. probe: the lanes that sit on a candidate end (the key's end, or a byte
//      before a `/`) probe the table in parallel and compare the key bytes
//      against the staged target;
//   5. the highest lane that matched holds the longest key: one ballot picks
//      it. Lane 0 writes the route row, the roster row's room word and, for a
//      miss under XYWS_RT_MISS_404, the accept row; lanes 0 .. 4 write the 404
//      in 16-byte lines (xyws_lines.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_lines.h"
#include "xyws_route.h"
#include "xyws_rows.h"

#define ROUTE_LANES 64u       // lanes per connection: one wave
#define ROUTE_STEP 4u         // target bytes per lane: 64 x 4 = XYWS_ROUTE_KEY_MAX
#define ROUTE_LINE 16u        // bytes a lane stages or writes
#define ROUTE_GRID_CAP 8192u  // 256 CUs x 32 one-wave workgroups; further connections are grid-strided
// The staged lines of xyws_routing::WINDOW bytes at any alignment.
#define ROUTE_STAGE (((15u + xyws_routing::WINDOW + 15u) >> 4) << 4)

static_assert(ROUTE_LANES * ROUTE_STEP == XYWS_ROUTE_KEY_MAX, "every byte of the key window has a lane");
static_assert(ROUTE_STAGE / ROUTE_LINE <= ROUTE_LANES && xyws_routing::RESP_404_LEN + 15u <= ROUTE_LINE * ROUTE_LANES,
              "one line per lane stages the window and writes the 404");

typedef __attribute__((address_space(3))) uint8_t l_u8;

using namespace xyws_internal;

// Target byte i is staged byte lo + i.
struct staged_target {
  const l_u8* s;
  XYWS_DEV uint8_t operator[](uint32_t i) const { return s[i]; }
};

__global__ void __launch_bounds__(ROUTE_LANES)
    k_route_streams(const xyws_accept_conn* __restrict__ aconns, xyws_accept_result* aresults,
                    const xyws_route_conn* __restrict__ rtconns, uint64_t n, const void* dev_table, uint64_t table_len,
                    xyws_roster_conn* rconns, uint64_t n_rconns, uint32_t default_room, uint32_t policy,
                    xyws_route_result* results) {
  __shared__ __attribute__((aligned(16))) uint8_t s_mem[ROUTE_STAGE];
  const uint32_t lane = threadIdx.x;
  xyws_routing::table tb = xyws_routing::open(dev_table, table_len);
  tb.slots = uniform32(tb.slots);
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const xyws_rows::accept_target at = xyws_rows::load_accept_target(aresults + ci);
    if (!(at.status & XYWS_ACC_ACCEPTED)) {  // rule 1
      if (lane == 0 && results)
        xyws_rows::store_route_result(results + ci, {XYWS_RT_NOT_ACCEPTED, XYWS_ROOM_NONE}, {xyws_routing::NO_ROUTE, 0}, 0);
      continue;
    }
    const xyws_rows::accept_conn_row cq = xyws_rows::load_accept_conn(aconns + ci);
    const uint32_t rconn = xyws_rows::load_route_conn(rtconns + ci);
    const uint64_t lim = cq.len < XYWS_ACCEPT_MAX_REQUEST ? cq.len : XYWS_ACCEPT_MAX_REQUEST;
    const bool trusted = (uint64_t)at.path_off + at.path_len <= lim;  // rule 4
    xyws_routing::found f = {0, XYWS_ROOM_NONE, xyws_routing::NO_ROUTE, 0};
    if (trusted) {
      // 1. the lines that hold the target's window
      const uint64_t src = cq.buf + at.path_off;
      const uint32_t lo = (uint32_t)(src & 15u);
      const uint32_t W = at.path_len < xyws_routing::WINDOW ? at.path_len : xyws_routing::WINDOW;
      const g_u8* const base = (const g_u8*)(src & ~15ull);
      const uint32_t nlines = W ? (lo + W + 15u) >> 4 : 0u;
      if (lane < nlines)
        *reinterpret_cast<u32x4*>(s_mem + ROUTE_LINE * lane) = *reinterpret_cast<const g_u32x4*>(base + ROUTE_LINE * lane);
      __syncthreads();
      const l_u8* const tgt = (const l_u8*)s_mem + lo;

      // 2. the key: this lane's bytes (those at or behind W are never used), the first `?` or `#`
      const uint32_t i0 = ROUTE_STEP * lane;
      uint32_t c[ROUTE_STEP + 1], mycut = 0xFFFFFFFFu;
#pragma unroll
      for (uint32_t t = 0; t <= ROUTE_STEP; t++) c[t] = tgt[i0 + t];  // (c[4]: the next lane's first, byte 256 for the last)
#pragma unroll
      for (uint32_t t = ROUTE_STEP; t-- > 0;)
        if (i0 + t < W && xyws_routing::ends_key(c[t])) mycut = i0 + t;
      const uint64_t cuts = __ballot(mycut != 0xFFFFFFFFu);
      uint32_t cut = 0xFFFFFFFFu;
      if (cuts) cut = (uint32_t)__shfl((int)mycut, __ffsll((unsigned long long)cuts) - 1);
      else if (W == xyws_routing::WINDOW && xyws_routing::ends_key(tgt[XYWS_ROUTE_KEY_MAX])) cut = XYWS_ROUTE_KEY_MAX;
      cut = uniform32(cut);
      uint32_t plen = xyws_routing::key_len_before_slash(at.path_len, cut);
      if (xyws_routing::slash_may_drop(plen, at.path_len) && tgt[plen - 1] == '/') plen--;
      plen = uniform32(plen);
      f.key_len = plen;

      if (tb.slots && plen) {
        // 3. the hash of the target up to this lane's first byte
        uint32_t inc = 0;
#pragma unroll
        for (uint32_t t = 0; t < ROUTE_STEP; t++) inc = xyws_routing::hash_step(inc, c[t]);
        uint32_t pw = xyws_routing::hash_pow(ROUTE_STEP);
#pragma unroll
        for (uint32_t d = 1; d < ROUTE_LANES; d <<= 1, pw *= pw) {
          const uint32_t below = (uint32_t)__shfl_up((int)inc, d);
          if (lane >= d) inc = xyws_routing::hash_join(below, inc, pw);
        }
        uint32_t h = (uint32_t)__shfl_up((int)inc, 1);
        if (lane == 0) h = 0;

        // 4. this lane's candidates, the shorter first
        const uint32_t first = tgt[0];
        const staged_target p = {tgt};
        uint32_t best = 0, room = XYWS_ROOM_NONE, route = xyws_routing::NO_ROUTE;
#pragma unroll
        for (uint32_t t = 0; t < ROUTE_STEP; t++) {
          const uint32_t j = i0 + t + 1;
          h = xyws_routing::hash_step(h, c[t]);
          bool exact;
          if (xyws_routing::is_candidate(j, plen, c[t + 1], first, exact) && xyws_routing::probe(tb, h, p, j, exact, room, route))
            best = j;
        }

        // 5. the highest lane that matched holds the longest key
        const uint64_t hits = __ballot(best != 0);
        if (hits) {
          const int win = 63 - __clzll((unsigned long long)hits);
          f.best = uniform32((uint32_t)__shfl((int)best, win));
          f.room = uniform32((uint32_t)__shfl((int)room, win));
          f.route = uniform32((uint32_t)__shfl((int)route, win));
        }
      }
      __syncthreads();  // (LDS is rewritten by the next connection)
    }
    uint32_t status = xyws_routing::match_status(tb, f) | (trusted ? 0u : XYWS_RT_BAD_ROW);
    uint32_t room = f.room;
    const bool miss = !(status & XYWS_RT_MATCHED);
    if (miss) xyws_routing::settle_miss(default_room, policy, status, room);
    if (!trusted) {  // its tables cannot be believed: the route row alone
      if (lane == 0 && results)
        xyws_rows::store_route_result(results + ci, {status, room}, {xyws_routing::NO_ROUTE, 0}, 0);
      continue;
    }
    if (rconn != XYWS_ROUTE_NO_ROW && rconn >= n_rconns) status |= XYWS_RT_BAD_ROW;

    if (miss && (policy & XYWS_RT_MISS_404)) {  // rule 3: response byte q at position olo + q from obase
      g_u8* const obase = (g_u8*)(cq.out & ~15ull);
      const uint64_t olo = cq.out & 15u;
      const uint64_t wlim = sat_add(olo, cq.out_cap), P1 = olo + xyws_routing::RESP_404_LEN;
      const uint64_t wl = P1 < wlim ? P1 : wlim;
      const uint64_t A = (uint64_t)ROUTE_LINE * lane;  // (64 + 15 bytes: one step)
      if (wl > olo && A < wl) {
        const uint64_t s = A > olo ? A : olo, e = A + 16 < P1 ? A + 16 : P1;
        bytes16 acc = {0, 0};
        for (uint32_t a = (uint32_t)(s - A), ae = (uint32_t)(e - A); a < ae; a++) {
          const uint64_t b = xyws_routing::resp_404((uint32_t)(A + a - olo));
          if (a < 8) acc.lo |= b << (8u * a);
          else acc.hi |= b << (8u * (a - 8));
        }
        put_line(obase, A, s, e, olo, wlim, acc);
      }
      if (lane == 0)
        xyws_rows::store_accept_result(
            aresults + ci, {XYWS_ACC_REJECTED | (xyws_routing::RESP_404_LEN > cq.out_cap ? XYWS_ACC_TRUNCATED : 0u), 404,
                            XYWS_ACR_NOT_FOUND, at.consumed, xyws_routing::RESP_404_LEN, 0, 0, 0xFFFFFFFFu});
    }
    if (lane == 0) {
      if (rconn != XYWS_ROUTE_NO_ROW && rconn < n_rconns) xyws_rows::store_roster_room(rconns + rconn, room);
      if (results)
        xyws_rows::store_route_result(results + ci, {status, room}, {f.route, at.path_off}, f.key_len);
    }
  }
}

extern "C" {

int xyws_route_streams(xyws_ctx* ctx, const xyws_accept_conn* dev_aconns, xyws_accept_result* dev_aresults,
                       const xyws_route_conn* dev_rtconns, uint64_t n, const void* dev_table, uint64_t table_len,
                       xyws_roster_conn* dev_rconns, uint64_t n_rconns, uint32_t default_room, uint32_t policy,
                       xyws_route_result* dev_results, void* stream) {
  if (!ctx || (n && (!dev_aconns || !dev_aresults || !dev_rtconns))) return XYWS_ERR_INVALID;
  if ((table_len && !dev_table) || (n_rconns && !dev_rconns) || !xyws_routing::args_ok(policy)) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, ROUTE_GRID_CAP);
  hipLaunchKernelGGL(k_route_streams, dim3(grid), dim3(ROUTE_LANES), 0, (hipStream_t)stream, dev_aconns, dev_aresults,
                     dev_rtconns, n, dev_table, table_len, dev_rconns, n_rconns, default_room, policy, dev_results);
  return hip_err(hipGetLastError());
}

int xyws_route_build(const xyws_route* routes, uint32_t n_routes, uint32_t slots, void* host_table, uint64_t cap,
                     uint64_t* need) {
  return xyws_routing::build(routes, n_routes, slots, host_table, cap, need);
}

int xyws_route_lookup(const void* host_table, uint64_t table_len, const void* target, uint64_t len,
                      xyws_route_result* res) {
  return xyws_routing::lookup_target(host_table, table_len, target, len, res);
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_route_streams. out: {lanes per connection, target bytes per lane, staged
// bytes per wave, grid cap}.
int xyws_debug_route_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = ROUTE_LANES;
  out[1] = ROUTE_STEP;
  out[2] = ROUTE_STAGE;
  out[3] = ROUTE_GRID_CAP;
  return XYWS_OK;
}

// Internal (tests, no HIP call): the slot at which the chain of a key in normal
// form begins in a table of `slots` slots, so that a test can choose keys that
// share one chain.
uint32_t xyws_debug_route_home(const void* key, uint32_t len, uint32_t slots) {
  uint32_t h = 0;
  for (uint32_t i = 0; i < len; i++) h = xyws_routing::hash_step(h, ((const uint8_t*)key)[i]);
  return xyws_routing::home(h, slots);
}

// Internal (measurements, no HIP call): xyws_route_lookup over the targets of n
// requests of one host slab, as their host accept rows name them, on the
// calling thread: what a caller without xyws_route_streams runs between its
// copies (scripts/route_rate.py). rooms[i]: the route's room, or default_room.
int xyws_debug_route_host(const void* host_table, uint64_t table_len, const void* host_reqs, uint64_t req_stride,
                          const xyws_accept_result* host_aresults, uint64_t n, uint32_t default_room, uint32_t* rooms) {
  if (n && (!host_reqs || !host_aresults || !rooms)) return XYWS_ERR_INVALID;
  for (uint64_t i = 0; i < n; i++) {
    xyws_route_result r;
    const int rc = xyws_routing::lookup_target(host_table, table_len,
                                             (const uint8_t*)host_reqs + req_stride * i + host_aresults[i].path_off,
                                             host_aresults[i].path_len, &r);
    if (rc) return rc;
    rooms[i] = r.status & XYWS_RT_MATCHED ? r.room : default_room;
  }
  return XYWS_OK;
}

}  // extern "C"
