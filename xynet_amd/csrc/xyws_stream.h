// xyws_stream.h — run-parallel stream decoder (xyws_stream.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xyws.h"
#include "xyws_host.h"

// ---------------------------------------------------------------- scratch layout
// The memory host and kernels share, described once: constants and asserts
// only, one constant per line with its value spelled out (xynet_amd/_lib.py
// mirrors them by name; tests/test_layout.py reads this section as text).

// Run scratch head: byte offsets. Zeroed at allocation.
constexpr uint32_t HEAD_TICKET = 0;   // u32: workgroups that have started in this call (reset by the finisher)
constexpr uint32_t HEAD_ERROR = 4;    // u32: the device error word (DERR_* bits), sticky until read back
constexpr uint32_t HEAD_TOTAL = 8;    // u64: frames of the last call
constexpr uint32_t HEAD_EPOCH = 16;   // u64: completed calls (a call runs with E = this + 1)
constexpr uint32_t HEAD_CARRY = 64;   // xyws_carry: run 0's snapshot of the incoming carry (64 bytes)
constexpr uint32_t HEAD_STATS = 128;  // u64 x XYWS_NSTATS: the debug stats (ST_* / LT_* slots)
constexpr uint32_t XYWS_NSTATS = 48;
// End-of-call words (u64 each), reset by the workgroup that finishes the call:
constexpr uint32_t HW_DONE = 512;       // workgroups done (counted in its low u32)
constexpr uint32_t HW_BAD = 520;        // != 0: a hand-over needs the repair walk
constexpr uint32_t HW_TOTAL = 528;      // frames of all items
constexpr uint32_t HW_FINAL = 536;      // final chain state of the item whose chain reached the batch end (5 words)
constexpr uint32_t HW_EMIT_SLOW = 584;  // descriptor emission: != 0 when the frame-start lists cannot be used (a region
                                        // overflowed, or a repaired hand-over changed the plan): k_stream_emit re-walks
constexpr uint32_t HW_EMIT_FLAG = 592;  // ...copied by finish_call for k_stream_emit (and reset there)
constexpr uint32_t HW_FSMAX = 600;      // decoder choice (plan_decode): the largest and
constexpr uint32_t HW_FSMIN = 608;      // ...complemented, the smallest last-frame size of the call's runs / segment exits
constexpr uint32_t HW_DPOL = 616;       // the device policy word (dpol_publish); not reset
constexpr uint32_t HEAD_BYTES = 1024;
static_assert(HEAD_CARRY + 64 <= HEAD_STATS && HEAD_STATS + 8 * XYWS_NSTATS <= HW_DONE, "head areas overlap");
static_assert(HW_FINAL + 5 * 8 <= HW_EMIT_SLOW && HW_DPOL + 8 <= HEAD_BYTES, "end-of-call words outside the head");

// Device error bits (xyws_ctx_last_device_error): the context's word (serial
// and indexed modes, the frames kernels) ORed with every scratch's HEAD_ERROR.
constexpr uint32_t DERR_TABLE = 0x1;     // serial scan: more frames than its table holds
constexpr uint32_t DERR_TIMEOUT = 0x2;   // run / lattice decoder: a bounded inter-workgroup wait timed out
constexpr uint32_t DERR_STALE = 0x4;     // run decoder: a run record was not written by its call
constexpr uint32_t DERR_TAG = 0x8;       // run decoder: a published entry granule with another call's tag (a torn read)
constexpr uint32_t DERR_SRC_OOB = 0x100; // frames kernels: a descriptor's payload lies past the source (read as zero)
constexpr uint32_t DERR_ORPHANS = 0x200; // xyws_reassemble: trailing continuation frames with no message after them

// Run record: R_WORDS x u64 per flat index (run r = 2r, its piece = 2r + 1).
enum {
  R_H = 0,        // prologue: entry,
  R_W = 1,        // write start,
  R_S0 = 2,       // entry state (5 words),
  R_HEAD = 7,     // head frames
  R_OKW = 8,      // results (OK_BIT, TMO_BIT): ok | tmo << 1 | succ << 32,
  R_HN = 9,       // the successor's entry as this run's chain met it,
  R_WN = 10,      // its write limit,
  R_CNT = 11,     // frames,
  R_TAIL = 12,    // frames at or past it,
  R_FIRST = 13,   // the first frame start at or past it
  R_F0 = 14,      // final state (5 words)
  R_EFROM = 20,   // emission plan (finish_call): first frame,
  R_ECNT = 21,    // count,
  R_EORD = 22,    // first ordinal,
  R_ECARRY = 23,  // the first one is the carried frame
  R_EP = 24,      // epoch of the call that wrote the results
  R_T0 = 25,      // stats mode: s_memrealtime at start,
  R_T1 = 26,      // after the prologue,
  R_T2 = 27,      // at the end
  R_SPLIT = 28,   // own runs: the split segment a thief took the rest from (NONE: none)
  R_XCC = 29,     // stats mode: the XCD (XCC_ID) the run's workgroup ran on
  R_NREC = 30,    // descriptors requested: frame starts in the item's region
  R_WORDS = 32
};
static_assert(R_S0 + 5 == R_HEAD && R_F0 + 5 < R_EFROM && R_NREC < R_WORDS, "run record words overlap");

// Run scratch placement for `units` runs (2 * units flat indices), as byte
// offsets:  head | entry granules (16 B per flat index) | split words (16 B per
// run) | progress words (8 B per run) | records. Everything below the
// records is zeroed at allocation (epoch 0: stale).
struct run_layout {
  uint64_t granules, split, prog, records;
  uint64_t zeroed, total;
};
inline run_layout run_layout_of(uint64_t units) {
  const auto pad = [](uint64_t bytes) { return (bytes + 255) & ~255ull; };
  run_layout l;
  l.granules = HEAD_BYTES;
  l.split = l.granules + pad(32 * units);
  l.prog = l.split + pad(16 * units);
  l.records = l.prog + pad(8 * units);
  l.zeroed = l.records;
  l.total = l.records + 2 * units * R_WORDS * 8;
  return l;
}

// Lattice scratch (xyws_lattice.h): u64 words, zeroed at allocation.
enum {
  LW_CNT = 0,         // u32 [0] claim counter, u32 [1] done count (reset by the finisher)
  LW_BRK = 2,         // ~(earliest failing lattice index) of this call, 0 = none (reset by the finisher)
  LW_UNMASK = 3,      // xyws_unmask's claim counter pair (u32 claims, u32 done; reset by its last workgroup)
  LW_W = 4,           // the decided prefix: every segment below it has published its result (reset by the finisher)
  LW_LOOPS = 5,       // workgroups whose segment loop has ended (reset by the finisher)
  LW_DPOL = 6,        // the device policy word of the previous call in the stream (dpol_publish: HW_DPOL's copy)
  LW_EPOCH = 7,       // completed calls (a call runs with E = this + 1)
  LW_REDIR = 8,       // redirect record for the run decoder: [0] state, [1] p, [2] frames before p
  LW_NBAIL_POL = 12,  // calls handed whole to the run decoder on the device policy word (cumulative)
  LW_NBAIL_HYP = 13,  // calls handed whole to the run decoder by the prologue's checks (cumulative)
  LW_NLOOP_A = 14,    // calls whose segment loops ran in the large-frame geometry (cumulative)
  LW_NLOOP_B = 15,    // ... in the default geometry (cumulative)
  LW_RCARRY = 16,     // the carry the run decoder starts from at p (8 words)
  LW_STAT = 32        // per segment: (E << 2) | LS_*
};
// the prologue loads {LW_DPOL, LW_EPOCH} in one round trip:
static_assert(LW_EPOCH == LW_DPOL + 1 && LW_DPOL % 2 == 0, "one 16-byte granule");

// Debug stats slots (XYWS_OPT_STATS, xyws_debug_stats). Slots 16..29 are
// shared: the run decoder's ST_* timing slots and the lattice decoder's LT_*
// phase clocks (the run decoder does not run in a call the lattice finished).
// Clocks are s_memtime ticks summed over workgroups.
enum {
  ST_RUNS = 0,         // runs
  ST_NONE = 1,         // runs without an entry
  ST_BAD = 2,          // hand-overs that needed the repair walk
  ST_REPAIR = 3,       // repairs
  ST_CUT = 4,          // chains whose next header crosses the write limit
  ST_SPIN = 5,         // sleeps spent waiting for another workgroup's word
  ST_SEGS = 6,         // dense passes
  ST_FRAMES = 7,       // frames
  ST_P_WIN = 8,        // entry scan: segments scanned,
  ST_P_CAND = 9,       // survivors of the filter,
  ST_P_UND = 10,       // chains undecided in their segment,
  ST_P_TCOMP = 11,     // clocks: filter,
  ST_P_TCHECK = 12,    // check,
  ST_P_TRES = 13,      // resolve
  ST_D_TENT = 14,      // dense pass: clocks of the entry speculation,
  ST_D_TCHASE = 15,    // of the sub-block chases
  ST_T_PRO = 16,       // run: clocks of the prologue,
  LT_C_A = 16,         // lattice, control lane: claim and entry, to barrier A
  ST_T_MAIN = 17,      // the main loop,
  LT_C_C = 17,         // publish and gate, to barrier C
  ST_T_WAIT = 18,      // the successor wait,
  LT_C_ADV = 18,       // after barrier D: advance, wait for A
  ST_T_FILL = 19,      // the LDS fill,
  LT_D_FILL = 19,      // lattice, data lane 64: LDS fill
  ST_T_CHASE = 20,     // the chase's barriers,
  LT_D_WB = 20,        // wait at barrier B
  ST_T_XOR = 21,       // the XOR and stores,
  LT_D_TAB = 21,       // frame table
  ST_T_TAIL = 22,      // the tail,
  LT_D_WC = 22,        // wait at barrier C
  ST_T_PF = 23,        // the prefetch issue,
  LT_D_MASK = 23,      // masks and XOR in LDS
  ST_T_CP = 24,        // the chase pass
  LT_D_WD = 24,        // wait at barrier D
  ST_P_FILL = 25,      // run prologue: clocks of its fill,
  LT_D_ST = 25,        // stores
  ST_P_SCAN = 26,      // its scan,
  LT_D_WA = 26,        // wait at barrier A
  ST_P_PUB = 27,       // its publish
  LT_SEGS = 27,        // lattice: segments (a count)
  ST_D_NOENT = 28,     // dense pass: sub-blocks without an entry,
  LT_GATE = 28,        // lattice, control lane: wait for its operations of a segment ago
  ST_D_CHASE = 29,     // whose chase failed,
  LT_END = 29,         // lattice: the first-segment gate's wait
  ST_D_MISMATCH = 30,  // that met another exit than speculated,
  ST_D_OVF = 31,       // passes whose frame list overflowed
  ST_GIVEUP = 32,      // runs that gave up on their successor
  ST_BRIDGE = 33,      // ...bridged by the finisher
  ST_STEAL_REQ = 34,   // work stealing: requests,
  ST_STEAL_ACC = 35,   // pieces taken,
  ST_STEAL_SEGS = 36,  // their segments
  ST_D_TVAL = 37,      // dense pass: clocks of the validation
  ST_T_ROWS = 38,      // run: clocks of the row table,
  ST_T_SER = 39,       // of the serial chase
  ST_P_LATTICE = 40,   // runs whose entry the lattice gave (find_entry)
  ST_X_W0 = 41,        // entry scan (lane 0), clocks: window 0 to its check,
  ST_X_BITS = 42,      // the rest's candidate bits (from the segment's start),
  ST_X_SURV = 43,      // its survivors loop
  ST_T_STRIDE = 46     // run: clocks of the stride pass
};
enum {
  LCLK_SLOT0 = 16,  // lat_clock's first slot
  LCLK_NSLOTS = 16  // ...and how many it flushes
};
static_assert(LT_C_A == LCLK_SLOT0 && LT_END < LCLK_SLOT0 + LCLK_NSLOTS && LCLK_SLOT0 + LCLK_NSLOTS <= ST_GIVEUP,
              "the lattice's clocks stay in the shared slots");
static_assert(ST_T_STRIDE < XYWS_NSTATS, "a stats slot outside the head's stats area");

// Pinned policy words (stream_scratch::pol_h; xyws_debug_policy, xyws_debug_plan).
enum {
  POL_EPOCH = 0,    // the call's epoch: written last (release), != 0 once a call has finished
  POL_BYTES = 1,    // batch bytes
  POL_FSMIN = 2,    // smallest last-frame size of the call's runs (0 with POL_FSMAX == 0: none)
  POL_FSMAX = 3,    // largest
  POL_DECODER = 4,  // DEC_*
  POL_WORDS = 5
};
// Decoder codes (POL_DECODER; bits 48..55 of the device policy word).
enum : uint64_t {
  DEC_RUNS = 0,     // the run decoder
  DEC_RUNS512 = 2,  // ...in 512-thread workgroups
  DEC_LATTICE = 3   // the lattice decoder held over the whole batch
};

// Scratch owned by a context: the run scratch (a head, and per run one
// record, entry granules, a split and a progress word), the descriptor
// regions and the lattice scratch; their words are laid out in the "scratch
// layout" section below. The three areas grow in reserve_for alone, from
// floors of SCRATCH_MIN_RUNS runs and SCRATCH_MIN_SEGS lattice segments.
constexpr uint64_t SCRATCH_MIN_RUNS = 64, SCRATCH_MIN_SEGS = 64;
struct stream_scratch {
  xyws_internal::dev_area runs;  // run scratch (units: runs)
  int ncu = 256;                 // compute units of the context's device (runs per launch)
  xyws_internal::dev_area desc;  // frame-start lists for descriptor emission (units: bytes, the caller's cap)
  // decoder choice: pinned host words the finisher of every call writes
  // (POL_*) and their device address; null when the pinned allocation failed (then the
  // run decoder serves every call)
  volatile uint64_t* pol_h = nullptr;
  uint64_t* pol_d = nullptr;
  xyws_internal::dev_area lat;   // lattice decoder: scratch words + one result word per segment (units: segments)
};

void stream_scratch_init(stream_scratch* s, int device);
void stream_scratch_free(stream_scratch* s);
// xyws_ctx_reserve: everything a decode of up to max_batch_bytes needs, and
// with max_frames its descriptor regions for that many frames (0: none)
int stream_scratch_reserve(stream_scratch* s, uint64_t max_batch_bytes, uint64_t max_frames);
// sticky device error word of this scratch (HEAD_ERROR: DERR_* bits); clear:
// reset it after reading (the device must be idle)
uint32_t stream_scratch_error(stream_scratch* s, bool clear);
int stream_scratch_stats(stream_scratch* s, uint64_t out[XYWS_NSTATS]);
int64_t stream_scratch_records(stream_scratch* s, uint64_t* out, uint64_t max_runs);
// {the device policy word (HW_DPOL), lattice calls handed whole to the run
// decoder on it, ... by the prologue's checks, lattice calls whose segment
// loops ran in 75 KiB segments, ... in 120 KiB segments}; synchronizes the
// device
int stream_scratch_lattice(stream_scratch* s, uint64_t out[5]);
// xyws_unmask's claim counter pair (u32 claims, u32 workgroups done; zeroed at
// allocation, reset by the kernel's last workgroup) in this scratch
int stream_scratch_unmask_counter(stream_scratch* s, bool capturing, uint32_t** out);

// Internal decode options (not part of include/xyws.h):
#define XYWS_OPT_WG256 0x8u  // the run decoder in four 256-thread workgroups per CU on 16 KiB segments
#define XYWS_OPT_TEST_LATSPEC 0x10u  // tests (lattice decoder): every store speculative (no first-segment gate, no
                                     // failing-point filter): a broken lattice is undone by the end-of-work check
#define XYWS_OPT_TEST_LATDUMP 0x20u  // tests (lattice decoder): a workgroup never undoes its own speculative
                                    // stores at its end: every list goes to the finisher
#define XYWS_OPT_LATX_NOWORK 0x40u  // timing experiment only (wrong bytes): the lattice decoder's data waves skip
                                    // the checks and the XOR (its data path and control alone)
#define XYWS_OPT_LATX_ONLY 0x80u  // timing experiment only (wrong bytes after a redirect): no run decoder after the lattice
#define XYWS_OPT_STATS 0x100u      // count speculation/repair events (xyws_debug_stats)
#define XYWS_OPT_SMALL_SEG 0x200u  // 1 KiB segments, one per run: exercises run-boundary
                                   // speculation and repair on small test inputs
#define XYWS_OPT_LATTICE 0x400u      // the lattice decoder first, whatever the decoder choice would take
#define XYWS_OPT_NO_LATDEC 0x800u    // never the lattice decoder
#define XYWS_OPT_NO_DENSE0 0x1000u  // experiment (run decoder): the stride pass first in every run's first
                                   // segment even after a call of small mixed-size frames (no dense0 hint)
#define XYWS_OPT_REDIRECT 0x2000u    // (set by launch_plan only) the run decoder after the lattice decoder:
                                     // it reads the lattice's redirect record first
#define XYWS_OPT_NO_LATENTRY 0x4000u // experiment (run decoder): no lattice entry (find_entry scans every run)
#define XYWS_OPT_WG1024 0x8000u    // the run decoder in its default geometry (one 1024-thread workgroup per CU),
                                   // whatever the geometry choice (wg512_preferred) would take
#define XYWS_OPT_RUNS_NOWAIT 0x10000u // experiment (run decoder): a serial-chase segment's stores do not wait for the
                                   // next segment's loads (the dense pass's behaviour)
#define XYWS_OPT_NO_STORE 0x20000u // diagnostics: decode without writing (timing split only)
#define XYWS_OPT_WG512 0x40000u    // two 512-thread workgroups per CU, 64 KiB segments
#define XYWS_OPT_DIAG 0x80000u     // diagnostics: no prefetch during the prologue scan (timing only)
#define XYWS_OPT_TEST_GIVEUP 0x100000u // tests: odd runs give up on their successor at once (the path
                                       // of a successor whose workgroup has not started; finish bridges it)
#define XYWS_OPT_NO_LATTICE 0x200000u   // experiment (run decoder): no lattice passes (row table and walk only)
#define XYWS_OPT_STEAL 0x400000u       // work stealing between runs (off by default: measured no faster on c1-c4)
#define XYWS_OPT_TEST_STEAL 0x800000u  // tests: stealing on, every fourth run starts late, pieces of 1 segment and up
#define XYWS_OPT_LAT_NOGATE 0x1000000u  // (set by the lattice kernel only, from the device policy word) no
                                        // first-segment gate: the previous call on the stream was the lattice's
#define XYWS_OPT_LAT_GATE 0x2000000u    // experiment (lattice decoder): the first-segment gate whatever the
                                        // previous call found
#define XYWS_OPT_BIGSCAN 0x4000000u  // tests (entry scans): one filter pass per segment, whatever the previous
                                     // call found
#define XYWS_OPT_LATX_NOCHK 0x8000000u  // experiment (lattice decoder): no check of lattice points 1 and 2 up front
#define XYWS_OPT_IOV_PIECES 0x10000000u  // xyws_decode_stream_iov: the pieces in place one by one (no descriptors)
#define XYWS_OPT_IOV_STAGE 0x20000000u   // xyws_decode_stream_iov: gather, decode, scatter whatever the pieces
#define XYWS_OPT_NO_BIGSCAN 0x40000000u // experiment (entry scans): the window-0 pass whatever the previous call found
#define XYWS_OPT_RUNS 0x80000000u     // the run decoder, whatever the decoder choice would take

// The stream decode's host side in three steps: plan_decode (pure: what the
// call will run and what scratch it needs), reserve_for (the only step that
// allocates, and the only one that fails with anything but XYWS_ERR_HIP),
// launch_plan (queues the kernels). A caller that queues several decodes
// (xyws_decode_stream_iov's pieces) plans them all and reserves their
// largest needs before it queues the first.

// The stream's previous call as the pinned policy words showed it at one
// moment: one snapshot per public call, every choice of the call from it. The
// device writes the words when a call finishes, so a snapshot may show any
// earlier call of the stream; it steers speed only (which decoder, which
// geometry, which entry scans go first), never the decode's result: every
// choice can be forced by an option, and the forced-option parity tests
// (tests/test_gpu_modes.py, test_gpu_lattice.py) hold each forced choice to
// the same bytes, descriptors and carry.
struct policy_view {
  bool present;    // the pinned words exist (else the run decoder serves every call)
  uint64_t epoch;  // != 0: a call has finished on this stream
  uint64_t fsmin, fsmax;  // smallest, largest last-frame size of that call's runs
};
policy_view policy_snapshot(const stream_scratch* s);

// What a decode needs of the three scratch areas (0: nothing).
struct scratch_need {
  uint64_t runs;        // run scratch, in runs
  uint64_t fmem_bytes;  // descriptor regions
  uint64_t lat_segs;    // lattice scratch, in segments
};
inline void need_max(scratch_need* a, const scratch_need& b) {
  if (b.runs > a->runs) a->runs = b.runs;
  if (b.fmem_bytes > a->fmem_bytes) a->fmem_bytes = b.fmem_bytes;
  if (b.lat_segs > a->lat_segs) a->lat_segs = b.lat_segs;
}

enum run_geom : uint32_t { GEOM_SMALL, GEOM_MID, GEOM_WG512, GEOM_PROD };
struct decode_plan {
  uint64_t lo, hi;     // the batch: bytes [lo, hi) from a 16-byte-aligned base
  uint32_t opts;       // (without XYWS_OPT_REDIRECT)
  run_geom geom;       // the run decoder's geometry, its segment bytes and threads
  uint32_t seg, threads;
  uint64_t nruns, rbytes;  // nruns == 0: an empty batch (k_stream_empty, no scratch)
  uint32_t nflat;
  bool want_lat;       // the lattice decoder first: lnseg segments of lseg[0] bytes, lgrid
  uint64_t lnseg;      // workgroups; the kernel takes lseg[0] or lseg[1] by the first frame
  uint32_t lgrid, lseg[2];
  uint64_t pfs;        // the run decoder's hints from the previous call (run_params)
  uint32_t dense0, bigscan;
  uint64_t rcap;       // entries per descriptor region (0: no descriptors)
  scratch_need need;
};
decode_plan plan_decode(int ncu, const policy_view& pv, uint64_t lo, uint64_t hi, uint64_t cap_if_frames,
                        uint32_t opts);
// The largest needs of any plan of a batch of up to max_batch_bytes with up to
// max_frames descriptors in the production geometries (the small-segment test
// mode grows lazily).
scratch_need plan_reserve(int ncu, uint64_t max_batch_bytes, uint64_t max_frames);
// capturing: XYWS_ERR_CAPACITY where an area would have to grow.
int reserve_for(stream_scratch* s, const scratch_need& need, bool capturing);
// After reserve_for(s, pl.need): fails with XYWS_ERR_HIP only.
int launch_plan(const stream_scratch* s, const decode_plan& pl, uint8_t* base, const xyws_carry* cin,
                xyws_carry* cout, xyws_frame* frames, uint64_t cap, uint64_t* nframes, hipStream_t stream);
// plan_decode, reserve_for, launch_plan
int stream_decode_fused(stream_scratch* s, uint8_t* base, uint64_t lo, uint64_t hi,
                        const xyws_carry* cin, xyws_carry* cout, xyws_frame* frames, uint64_t cap,
                        uint64_t* nframes, uint32_t opts, hipStream_t stream);
