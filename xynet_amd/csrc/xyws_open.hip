// xyws_open.hip — xyws_open_streams: rooms opened on the device for request
// paths that no route serves. The candidates among a sweep's route rows are
// looked up in, and inserted into, a device-resident hash table (the room
// directory) by three launches in stream order. The semantics are stated in
// include/xyws.h, the blob and its probe at rest in xyws_directory.h; this is
// how the device inserts concurrently and still numbers what it inserted the
// same way every time.
//
//   1. k_open_find: one wave per row, rows grid-strided. The wave stages the
//      16-byte lines that hold the row's key into LDS, hashes it (four bytes a
//      lane, one wave scan of six shuffle steps over hash_join: the route
//      kernel's scan, restated because only the whole key's hash is wanted
//      here), and walks the chain from home(hash):
//        USED     a key of an earlier call: hash, length, then the arena's
//                 bytes against the staged key, four bytes a lane;
//        PENDING  claimed in this launch by row `claimer`: compared against
//                 the claimer's *request bytes*, which its route row and its
//                 accept table row name and which nobody writes during the
//                 call. So no wave ever waits for another to publish anything;
//        EMPTY    lane 0 claims it with one 64-bit compare-and-swap of
//                 {state, claimer}: {EMPTY, *} -> {PENDING, k}. A failed swap
//                 looks at the same slot again, which is PENDING now;
//        DEAD     walked past.
//      Slots only ever leave EMPTY, so a wave meets the slot of its key before
//      the first EMPTY one and a key gets one slot. On its key's slot the wave
//      lowers slot.first to its row with atomicMin. The state word is read with
//      a device-scope atomic load; everything is vector atomics and vector
//      stores. The verdict goes to dev_work[k]: {tag, room or slot, hash,
//      key_len}. A closed directory, or one with fewer free slots than the call
//      has rows (xyws_directory.h), is only searched.
//   2. k_open_number: one workgroup of 1024 threads, ceil(n / 1024) rounds. Row
//      k is the first of a new key iff its verdict is PENDING and
//      slot.first == k: the flags come from the slots, no list and no counter
//      has to be cleared between calls. An exclusive scan of {1, key_len} over
//      the rows in index order (wave scans, the sixteen wave totals through
//      LDS, a running carry between rounds) numbers the keys; the thread of a
//      first row writes room (or XYWS_ROOM_NONE: refused), key_off, key_len
//      and hash into its slot. Thread 0 advances n_open, keys_used and dead.
//   3. k_open_commit: one wave per row. Every PENDING row takes its room from
//      its slot; the first row also copies the key from its request into the
//      arena (copy_span, xyws_lines.h: neighbouring keys share 16-byte lines)
//      and turns the slot USED, or DEAD for a refused key. Every candidate
//      writes its route row's place word and its roster row's room word
//      through xyws_rows.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_lines.h"
#include "xyws_route.h"
#include "xyws_directory.h"
#include "xyws_rows.h"

#define OPEN_LANES 64u        // lanes per row: one wave
#define OPEN_STEP 4u          // key bytes per lane: 64 x 4 = XYWS_ROUTE_KEY_MAX
#define OPEN_LINE 16u         // bytes a lane stages or copies
#define OPEN_GRID_CAP 8192u   // the route kernel's: 256 CUs x 32 one-wave workgroups; further rows are grid-strided
#define OPEN_SCAN 1024u       // threads of the numbering workgroup: rows per round
#define OPEN_STAGE (((15u + XYWS_ROUTE_KEY_MAX + 15u) >> 4) << 4)  // the lines of a key at any alignment

static_assert(OPEN_LANES * OPEN_STEP == XYWS_ROUTE_KEY_MAX, "every byte of a key has a lane");
static_assert(OPEN_STAGE / OPEN_LINE <= OPEN_LANES, "one line per lane stages a key");
static_assert(XYWS_OPEN_WORK_WORDS == 4, "dev_work: tag, value, hash, key_len");

typedef __attribute__((address_space(3))) uint8_t l_u8;

using namespace xyws_internal;
namespace D = xyws_directory;

// dev_work[k]: what the launches hand each other about row k.
enum : uint32_t { W_TAG = 0, W_VALUE = 1, W_HASH = 2, W_KEY_LEN = 3 };
enum : uint32_t {
  T_NONE = 0,       // no candidate: nothing is written for the row
  T_FOUND = 1,      // value: the room the directory holds for the key
  T_PENDING = 2,    // value: the slot claimed for the key in this call
  T_FULL = 3,       // no room left
  T_BAD_ROW = 4,    // the key lies outside the request
  T_BAD_TABLE = 5,  // the bytes are no directory
};

XYWS_DEV bool is_candidate(const xyws_rows::route_row& r, uint32_t from_room) {
  const bool by = (r.status & XYWS_RT_MISS) ||
                  (r.status & (XYWS_RT_MATCHED | XYWS_RT_BY_PREFIX)) == (XYWS_RT_MATCHED | XYWS_RT_BY_PREFIX);
  return r.room == from_room && by && !(r.status & (XYWS_RT_NOT_FOUND | XYWS_RT_NOT_ACCEPTED | XYWS_RT_BAD_ROW)) &&
         r.key_len >= 1 && r.key_len <= XYWS_ROUTE_KEY_MAX;
}
XYWS_DEV bool is_trusted(const xyws_rows::route_row& r, const xyws_rows::accept_recv& q) {
  const uint64_t lim = q.len < XYWS_ACCEPT_MAX_REQUEST ? q.len : XYWS_ACCEPT_MAX_REQUEST;
  return (uint64_t)r.key_off + r.key_len <= lim;
}

// Whether the len key bytes at the device address g equal the staged key: lane l compares bytes 4l .. 4l + 3.
XYWS_DEV bool same_key(const l_u8* key, uint64_t g, uint32_t len, uint32_t lane) {
  bool differ = false;
#pragma unroll
  for (uint32_t t = 0; t < OPEN_STEP; t++) {
    const uint32_t j = OPEN_STEP * lane + t;
    if (j < len) differ |= ((const g_u8*)g)[j] != key[j];
  }
  return __ballot(differ) == 0;
}

__global__ void __launch_bounds__(OPEN_LANES)
    k_open_find(const xyws_accept_conn* __restrict__ aconns, uint64_t n, void* dev_directory, uint64_t directory_len,
                uint32_t from_room, const xyws_route_result* results, uint32_t* work) {
  __shared__ __attribute__((aligned(16))) uint8_t s_mem[OPEN_STAGE];
  const uint32_t lane = threadIdx.x;
  // (plain loads: the header is written by k_open_number only, in stream order behind this launch, and two calls
  // over one directory never run concurrently, so every wave of the launch sees the same header)
  D::dir d = D::open(dev_directory, directory_len);
  d.slots = uniform32(d.slots);
  const bool shut = d.bad || !D::may_claim(d, n);
  g_u8* const blob = (g_u8*)dev_directory;
  for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
    const xyws_rows::route_row r = xyws_rows::load_route_row(results + k);
    uint32_t tag = T_NONE, value = 0, h = 0;
    if (is_candidate(r, from_room)) {
      const xyws_rows::accept_recv q = xyws_rows::load_accept_recv(aconns + k);
      if (!is_trusted(r, q)) tag = T_BAD_ROW;
      else if (d.bad) tag = T_BAD_TABLE;
      else {
        // the lines that hold the key
        const uint64_t src = q.buf + r.key_off;
        const uint32_t lo = (uint32_t)(src & 15u);
        const g_u8* const base = (const g_u8*)(src & ~15ull);
        if (lane < (lo + r.key_len + 15u) >> 4)
          *reinterpret_cast<u32x4*>(s_mem + OPEN_LINE * lane) = *reinterpret_cast<const g_u32x4*>(base + OPEN_LINE * lane);
        __syncthreads();
        const l_u8* const key = (const l_u8*)s_mem + lo;

        // the key's hash: each lane's four bytes, a scan over the lanes, the last byte's lane finishes
        const uint32_t i0 = OPEN_STEP * lane;
        uint32_t c[OPEN_STEP], inc = 0;
#pragma unroll
        for (uint32_t t = 0; t < OPEN_STEP; t++) c[t] = key[i0 + t];  // (those at or behind key_len are never used)
#pragma unroll
        for (uint32_t t = 0; t < OPEN_STEP; t++) inc = xyws_routing::hash_step(inc, c[t]);
        uint32_t pw = xyws_routing::hash_pow(OPEN_STEP);
#pragma unroll
        for (uint32_t s = 1; s < OPEN_LANES; s <<= 1, pw *= pw) {
          const uint32_t below = (uint32_t)__shfl_up((int)inc, s);
          if (lane >= s) inc = xyws_routing::hash_join(below, inc, pw);
        }
        uint32_t hl = (uint32_t)__shfl_up((int)inc, 1);
        if (lane == 0) hl = 0;
#pragma unroll
        for (uint32_t t = 0; t < OPEN_STEP; t++)
          if (i0 + t < r.key_len) hl = xyws_routing::hash_step(hl, c[t]);
        h = uniform32((uint32_t)__shfl((int)hl, (int)((r.key_len - 1) / OPEN_STEP)));

        // the chain
        tag = T_FULL;
        uint32_t i = D::home(h, d.slots);
        for (uint32_t step = 0; step < d.slots; step++, i = (i + 1) & (d.slots - 1)) {
          g_u8* const slot = blob + D::slot_at(i);
          unsigned long long* const claim = (unsigned long long*)(uint8_t*)(slot + D::S_STATE);
          uint32_t* const first = (uint32_t*)(uint8_t*)(slot + D::S_FIRST);
          uint64_t w = uniform64(__hip_atomic_load(claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          if ((uint32_t)w == D::EMPTY) {
            if (shut) break;
            uint64_t old = 0;
            if (lane == 0) old = atomicCAS(claim, w, (uint64_t)D::PENDING | ((uint64_t)(uint32_t)k << 32));
            old = uniform64(old);
            if (old == w) {
              if (lane == 0) atomicMin(first, (uint32_t)k);
              tag = T_PENDING;
              value = i;
              break;
            }
            w = old;  // somebody else's now: PENDING, with this key or another
          }
          const uint32_t state = (uint32_t)w;
          if (state == D::PENDING) {
            const uint32_t cl = (uint32_t)(w >> 32);
            if (cl >= n) continue;  // (a damaged blob)
            const xyws_rows::route_row cr = xyws_rows::load_route_row(results + cl);
            if (cr.key_len != r.key_len || !is_candidate(cr, from_room)) continue;  // (a claimer was a candidate)
            const xyws_rows::accept_recv cq = xyws_rows::load_accept_recv(aconns + cl);
            if (!is_trusted(cr, cq) || !same_key(key, cq.buf + cr.key_off, r.key_len, lane)) continue;
            if (lane == 0) atomicMin(first, (uint32_t)k);
            tag = T_PENDING;
            value = i;
            break;
          }
          if (state == D::USED) {
            const u32x4 f = *reinterpret_cast<const g_u32x4*>(slot + D::S_HASH);  // hash, key_off, key_len, room
            const uint32_t sh = uniform32(f.x), ko = uniform32(f.y), kl = uniform32(f.z), room = uniform32(f.w);
            if (sh != h || kl != r.key_len || !D::slot_ok(d, ko, kl, room)) continue;
            if (!same_key(key, (uint64_t)(blob + ko), kl, lane)) continue;
            tag = T_FOUND;
            value = room;
            break;
          }
        }
        __syncthreads();  // (LDS is rewritten by the next row)
      }
    }
    if (lane < XYWS_OPEN_WORK_WORDS)
      work[XYWS_OPEN_WORK_WORDS * k + lane] = lane == W_TAG ? tag : lane == W_VALUE ? value : lane == W_HASH ? h : r.key_len;
  }
}

// An exclusive scan of {c, b} over the workgroup's threads in thread order; the totals in tc, tb.
XYWS_DEV void scan_rows(uint32_t c, uint64_t b, uint32_t* s_c, uint64_t* s_b, uint32_t& ec, uint64_t& eb, uint32_t& tc,
                        uint64_t& tb) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t ic = c;
  uint64_t ib = b;
#pragma unroll
  for (uint32_t s = 1; s < 64; s <<= 1) {
    const uint32_t uc = (uint32_t)__shfl_up((int)ic, s);
    const uint64_t ub = (uint64_t)__shfl_up((long long)ib, s);
    if (lane >= s) {
      ic += uc;
      ib += ub;
    }
  }
  if (lane == 63) {
    s_c[wave] = ic;
    s_b[wave] = ib;
  }
  __syncthreads();
  ec = ic - c;
  eb = ib - b;
  tc = 0;
  tb = 0;
#pragma unroll
  for (uint32_t w = 0; w < OPEN_SCAN / 64; w++) {
    if (w < wave) {
      ec += s_c[w];
      eb += s_b[w];
    }
    tc += s_c[w];
    tb += s_b[w];
  }
  __syncthreads();  // (the totals are rewritten by the next round)
}

__global__ void __launch_bounds__(OPEN_SCAN)
    k_open_number(uint64_t n, void* dev_directory, uint64_t directory_len, const uint32_t* work) {
  __shared__ uint32_t s_c[OPEN_SCAN / 64];
  __shared__ uint64_t s_b[OPEN_SCAN / 64];
  __shared__ uint32_t s_admitted;            // the admitted keys are a prefix of the order: the highest ordinal + 1
  __shared__ unsigned long long s_kept;      // and the highest arena end among them
  const D::dir d = D::open(dev_directory, directory_len);
  if (d.bad) return;  // (nothing was claimed)
  g_u8* const blob = (g_u8*)dev_directory;
  uint32_t seen = 0;   // new keys before this round
  uint64_t bytes = 0;  // their summed lengths
  if (threadIdx.x == 0) {
    s_admitted = 0;
    s_kept = 0;
  }
  __syncthreads();  // (and every thread has read the header before thread 0 rewrites it)
  for (uint64_t k0 = 0; k0 < n; k0 += OPEN_SCAN) {
    const uint64_t k = k0 + threadIdx.x;
    uint32_t is_first = 0, len = 0, h = 0;
    g_u8* slot = nullptr;
    if (k < n && work[XYWS_OPEN_WORK_WORDS * k + W_TAG] == T_PENDING) {
      const uint32_t i = work[XYWS_OPEN_WORK_WORDS * k + W_VALUE];
      if (i < d.slots) {
        slot = blob + D::slot_at(i);
        is_first = *(const XYWS_GLOBAL uint32_t*)(slot + D::S_FIRST) == (uint32_t)k;
        h = work[XYWS_OPEN_WORK_WORDS * k + W_HASH];
        len = is_first ? work[XYWS_OPEN_WORK_WORDS * k + W_KEY_LEN] : 0u;
      }
    }
    uint32_t ec, tc;
    uint64_t eb, tb;
    scan_rows(is_first, len, s_c, s_b, ec, eb, tc, tb);
    if (is_first) {
      const uint64_t ord = (uint64_t)d.n_open + seen + ec, end = (uint64_t)d.keys_used + bytes + eb + len;
      const bool ok = ord < d.room_cap && end <= d.keys_cap;
      XYWS_GLOBAL uint32_t* const f = (XYWS_GLOBAL uint32_t*)slot;
      f[D::S_HASH / 4] = h;
      f[D::S_KEY_OFF / 4] = ok ? (uint32_t)(d.keys_off + end - len) : 0u;
      f[D::S_KEY_LEN / 4] = len;
      f[D::S_ROOM / 4] = ok ? d.room_base + (uint32_t)ord : XYWS_ROOM_NONE;
      if (ok) {
        atomicMax(&s_admitted, seen + ec + 1u);
        atomicMax(&s_kept, (unsigned long long)(bytes + eb + len));
      }
    }
    seen += tc;
    bytes += tb;
  }
  __syncthreads();
  if (threadIdx.x == 0 && seen) {
    XYWS_GLOBAL uint32_t* const hd = (XYWS_GLOBAL uint32_t*)blob;
    hd[D::H_N_OPEN / 4] = d.n_open + s_admitted;
    hd[D::H_KEYS_USED / 4] = d.keys_used + (uint32_t)s_kept;
    hd[D::H_DEAD / 4] = d.dead + (seen - s_admitted);
  }
}

__global__ void __launch_bounds__(OPEN_LANES)
    k_open_commit(const xyws_accept_conn* __restrict__ aconns, const xyws_route_conn* __restrict__ rtconns, uint64_t n,
                  void* dev_directory, uint64_t directory_len, xyws_roster_conn* rconns, uint64_t n_rconns,
                  uint32_t from_room, xyws_route_result* results, const uint32_t* work) {
  const uint32_t lane = threadIdx.x;
  D::dir d = D::open(dev_directory, directory_len);
  d.slots = uniform32(d.slots);
  g_u8* const blob = (g_u8*)dev_directory;
  for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
    const uint32_t tag = uniform32(work[XYWS_OPEN_WORK_WORDS * k + W_TAG]);
    if (tag == T_NONE) continue;
    const xyws_rows::route_row r = xyws_rows::load_route_row(results + k);
    if (tag == T_BAD_ROW) {  // its tables cannot be believed: the route row alone
      if (lane == 0) xyws_rows::store_route_place(results + k, {r.status | XYWS_RT_BAD_ROW, r.room});
      continue;
    }
    const uint32_t value = uniform32(work[XYWS_OPEN_WORK_WORDS * k + W_VALUE]);
    uint32_t status = r.status, room = from_room;
    if (tag == T_FOUND) {
      status |= XYWS_RT_DIRECTORY;
      room = value;
    } else if (tag == T_PENDING && !d.bad && value < d.slots) {
      g_u8* const slot = blob + D::slot_at(value);
      const u32x4 f = *reinterpret_cast<const g_u32x4*>(slot + D::S_HASH);  // hash, key_off, key_len, room
      const uint32_t ko = uniform32(f.y), kl = uniform32(f.z), sroom = uniform32(f.w);
      const bool mine = uniform32(*(const XYWS_GLOBAL uint32_t*)(slot + D::S_FIRST)) == (uint32_t)k;
      const bool ok = sroom != XYWS_ROOM_NONE && kl == r.key_len && ko >= d.keys_off &&
                      (uint64_t)ko + kl <= (uint64_t)d.keys_off + d.keys_cap;
      if (ok) {
        status |= XYWS_RT_OPENED;
        room = sroom;
      } else {
        status |= XYWS_RT_DIR_FULL;
      }
      if (mine) {
        if (ok) {
          const xyws_rows::accept_recv q = xyws_rows::load_accept_recv(aconns + k);
          const uint64_t dst = (uint64_t)(blob + ko);
          copy_span((g_u8*)(dst & ~15ull), dst & 15u, (dst & 15u) + kl, q.buf + r.key_off, 0, OPEN_LINE * OPEN_LANES, lane);
        }
        if (lane == 0) *(XYWS_GLOBAL uint32_t*)(slot + D::S_STATE) = ok ? D::USED : D::DEAD;
      }
    } else {
      status |= XYWS_RT_DIR_FULL | (tag == T_BAD_TABLE || d.bad ? XYWS_RT_BAD_TABLE : 0u);
    }
    const uint32_t rconn = xyws_rows::load_route_conn(rtconns + k);
    if (rconn != XYWS_ROUTE_NO_ROW && rconn >= n_rconns) status |= XYWS_RT_BAD_ROW;
    if (lane == 0) {
      if (rconn != XYWS_ROUTE_NO_ROW && rconn < n_rconns) xyws_rows::store_roster_room(rconns + rconn, room);
      xyws_rows::store_route_place(results + k, {status, room});
    }
  }
}

extern "C" {

int xyws_open_streams(xyws_ctx* ctx, const xyws_accept_conn* dev_aconns, const xyws_route_conn* dev_rtconns, uint64_t n,
                      void* dev_directory, uint64_t directory_len, xyws_roster_conn* dev_rconns, uint64_t n_rconns,
                      uint32_t from_room, xyws_route_result* dev_results, uint32_t* dev_work, void* stream) {
  if (!ctx || !dev_directory || !directory_len || (n_rconns && !dev_rconns) || n >= 0xFFFFFFFFull) return XYWS_ERR_INVALID;
  if (n && (!dev_aconns || !dev_rtconns || !dev_results || !dev_work)) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, OPEN_GRID_CAP);
  hipLaunchKernelGGL(k_open_find, dim3(grid), dim3(OPEN_LANES), 0, (hipStream_t)stream, dev_aconns, n, dev_directory,
                     directory_len, from_room, dev_results, dev_work);
  hipLaunchKernelGGL(k_open_number, dim3(1), dim3(OPEN_SCAN), 0, (hipStream_t)stream, n, dev_directory, directory_len,
                     dev_work);
  hipLaunchKernelGGL(k_open_commit, dim3(grid), dim3(OPEN_LANES), 0, (hipStream_t)stream, dev_aconns, dev_rtconns, n,
                     dev_directory, directory_len, dev_rconns, n_rconns, from_room, dev_results, dev_work);
  return hip_err(hipGetLastError());
}

int xyws_directory_init(uint32_t slots, uint32_t room_base, uint32_t room_cap, uint32_t keys_cap, void* host_blob,
                        uint64_t cap, uint64_t* need) {
  return D::init(slots, room_base, room_cap, keys_cap, host_blob, cap, need);
}

int xyws_directory_lookup(const void* host_blob, uint64_t len, const void* key, uint32_t key_len, uint32_t* room) {
  return D::lookup(host_blob, len, key, key_len, room);
}

int xyws_directory_get(const void* host_blob, uint64_t len, uint32_t from, uint32_t* key_off, uint32_t* key_len,
                       uint32_t* room, uint32_t* next) {
  return D::get(host_blob, len, from, key_off, key_len, room, next);
}

int xyws_directory_stat(const void* host_blob, uint64_t len, xyws_directory_info* info) {
  return D::stat(host_blob, len, info);
}

// Internal (tests and measurements, no HIP call): the geometry of the three
// kernels. out: {lanes per row, key bytes per lane, threads (rows per round) of
// the numbering workgroup, grid cap}.
int xyws_debug_open_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = OPEN_LANES;
  out[1] = OPEN_STEP;
  out[2] = OPEN_SCAN;
  out[3] = OPEN_GRID_CAP;
  return XYWS_OK;
}

// Internal (tests, no HIP call): the slot at which the chain of a key begins in
// a directory of `slots` slots, so that a test can choose keys that share one
// chain.
uint32_t xyws_debug_directory_home(const void* key, uint32_t len, uint32_t slots) {
  uint32_t h = 0;
  for (uint32_t i = 0; i < len; i++) h = D::hash_step(h, ((const uint8_t*)key)[i]);
  return D::home(h, slots);
}

}  // extern "C"
