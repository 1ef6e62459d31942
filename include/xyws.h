/*
 * xyws.h — C-ABI of the MI355X (gfx950) WebSocket frame-decode path.
 *
 * This is the drop-in boundary that replaces the CPU hot path of xynet's
 * WebSocket layer (paths relative to the xynet reference tree):
 *
 *   reference symbol                                         replaced by
 *   -------------------------------------------------------  ---------------------------
 *   websocket_mask(R&&, uint32_t mask, size_t i) -> size_t   xyws_unmask
 *     include/xynet/http/websocket_frame_mask.h:6-25
 *   websocket_frame_header_parser::parse / result / reset    xyws_decode_stream (parse
 *     include/xynet/http/websocket_frame_header.h:226-385      state carried in xyws_carry)
 *   websocket_recv_data: parse -> result -> websocket_mask   xyws_decode_stream,
 *     example/include/common/websocket.h:110-134               xyws_decode_indexed
 *   the websocket_recv_data loop of every connection, run    xyws_decode_streams (the recv
 *     once per coroutine                                       buffers of many connections,
 *     example/include/common/websocket.h:110-134               one launch)
 *   enum class websocket_flags                               XYWS_FLAG_* (same encoding)
 *     include/xynet/http/websocket_frame_header.h:42-58
 *   websocket_frame_header_parser (incremental, one header)  xyws_parser_* (runs the stream
 *     include/xynet/http/websocket_frame_header.h:226-385      decoder in parse-only mode)
 *   detail::websocket_frame_header_builder                   xyws_header_build (one header),
 *     include/xynet/http/websocket_frame_header.h:136-175      xyws_encode_frames (batched, device)
 *   echo_once: header{FIN|TEXT, len} + send(header, data)    xyws_encode_frames (one connection),
 *     example/websocket/websocket_echo.cpp:18-27               xyws_reply_streams (many)
 *   websocket_check_parser_result (close policy)             xyws_classify_frames (one connection),
 *     example/include/common/websocket.h:81-108                xyws_reply_streams (many)
 *   websocket_send_close: header{FIN|CLOSE, 2} + code        xyws_reply_streams (the close frame
 *     example/include/common/websocket.h:70-76                 ends the connection's reply)
 *   websocket_echo's loop: recv_data, check, echo_once or    xyws_decode_streams, then
 *     send_close, once per coroutine                           xyws_reply_streams: two launches
 *     example/websocket/websocket_echo.cpp:29-50               for a whole sweep
 *   (new) FIN=0 message reassembly + UTF-8 validation        xyws_reassemble (one batch),
 *                                                              xyws_reassemble_stream (messages, frames
 *                                                              and UTF-8 sequences cut by a recv
 *                                                              boundary, state in xyws_msg_carry)
 *   chat session's receive loop: one text message per        xyws_reassemble_streams (every
 *     connection and sweep, handed on to the room              connection's messages, one launch,
 *     example/websocket/websocket_chat.cpp:177-200             after xyws_decode_streams)
 *   chat_room::deliver + chat_session::writer: each message  xyws_broadcast_streams (a room's
 *     framed and sent once per member                          messages framed once, the wire
 *     example/websocket/websocket_chat.cpp:89-101, 148-175     copied to every member's send range)
 *   (new) a chat message cut by a recv boundary, which the   xyws_hold_streams (its parts kept
 *     reference's session reads to its end before deliver      on the device between sweeps, the
 *     example/websocket/websocket_chat.cpp:177-200              whole message handed to the room)
 *   chat_room::join + deliver_recent_messages: the last 10    xyws_backlog_streams (each room's
 *     messages (m_recent_messages) sent to a newcomer           newest frames kept in a log on the
 *     example/websocket/websocket_chat.cpp:34-47, 89-95         device, copied behind a joiner's send bytes)
 *   websocket_request_handler (parse, generate_response)     xyws_accept_streams (the opening
 *     include/xynet/http/websocket_request_handler.h           handshakes of many connections, one
 *     as websocket_handshake runs it, once per coroutine       launch), xyws_accept_request (one
 *     example/include/common/websocket.h:40-68                 request in host memory)
 *   websocket_request_handler::get_path, which a server      xyws_route_streams (each accepted
 *     with several rooms looks up on the host                  connection's room from its request
 *     include/xynet/http/websocket_request_handler.h           target, one launch), xyws_route_lookup
 *   recv_all / io_service remote-queue eventfd               xyws_arena_* (pinned recv arena,
 *     include/xynet/socket/impl/recv_all.h:86-121              H2D -> decode -> D2H, completion
 *     include/xynet/io_service.h:362-381                       written to an eventfd)
 *
 * The reference has no FFI of its own: it is a header-only C++20 library whose
 * templates are instantiated in the caller's translation unit. A caller (an
 * io_uring/coroutine service in the xynet style) keeps its sockets and
 * buffer_sequence unchanged and hands device-resident recv buffers to these
 * entry points; see INTEGRATION.md for the binding a maintainer would add.
 *
 * Conventions
 *   - Plain C types only. Device pointers are void* / typed pointers into
 *     device memory (hipMalloc or equivalent); `stream` is a hipStream_t passed
 *     as void* (NULL = the legacy default stream).
 *   - Every call is asynchronous on `stream` and returns an int status
 *     (XYWS_OK or a negative XYWS_ERR_*). Device-side results (frame tables,
 *     frame counts, carries) are valid once the stream reaches the call.
 *   - Buffers are owned by the caller. Unmasking mutates the caller's buffer in
 *     place, exactly like websocket_mask (websocket_frame_mask.h:16). The
 *     context owns only its scratch (tile status records, frame tables).
 *   - Parse semantics are the reference's, bit for bit: nothing is rejected
 *     (RSV bits, reserved opcodes, non-minimal or 2^63+ lengths are accepted,
 *     websocket_frame_header.h:305-385); violations are only *reported* in
 *     xyws_frame.status. An unmasked frame has key 0 (the parser's m_mask after
 *     reset(), :274-281), so its payload is left unchanged.
 *   - No CPU fallback: every entry point that computes runs HIP kernels for
 *     gfx950; if no device is present the call fails with XYWS_ERR_HIP.
 */
#ifndef XYWS_H
#define XYWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XYWS_ABI_VERSION 2

/* ---- status codes -------------------------------------------------------- */
#define XYWS_OK              0
#define XYWS_ERR_INVALID    -1  /* bad argument (null ctx, misaligned length, ...) */
#define XYWS_ERR_HIP        -2  /* a HIP runtime call failed (no device, launch error) */
#define XYWS_ERR_NOMEM      -3  /* device scratch allocation failed */
#define XYWS_ERR_CAPACITY   -4  /* batch larger than xyws_ctx_reserve() allowed while capturing */
#define XYWS_ERR_DEVICE     -5  /* a device-side bound tripped (see xyws_ctx_last_device_error) */
#define XYWS_ERR_AGAIN      -6  /* not complete yet (xyws_arena_poll) / no free slot (xyws_arena_submit) */

/* ---- websocket_flags encoding (websocket_frame_header.h:42-58) ----------- */
#define XYWS_FLAG_OP_CONTINUE 0x00
#define XYWS_FLAG_OP_TEXT     0x01
#define XYWS_FLAG_OP_BINARY   0x02
#define XYWS_FLAG_OP_CLOSE    0x08
#define XYWS_FLAG_OP_PING     0x09
#define XYWS_FLAG_OP_PONG     0x0A
#define XYWS_FLAG_OP_MASK     0x0F
#define XYWS_FLAG_FIN         0x10
#define XYWS_FLAG_HAS_MASK    0x20

/* Largest header: calc_frame_header_size(WS_HAS_MASK, UINT32_MAX)
 * (websocket_frame_header.h:111-134). */
#define XYWS_MAX_FRAME_HEADER_SIZE 14

/* ---- per-frame status bits (informational; never change the output) ----- */
#define XYWS_ST_PAYLOAD_INCOMPLETE 0x01 /* payload runs past the batch end (continues in carry) */
#define XYWS_ST_RSV                0x02 /* RSV1..3 set (parser drops them, :315) */
#define XYWS_ST_RESERVED_OPCODE    0x04 /* opcode 3-7 or 11-15 */
#define XYWS_ST_NONMINIMAL_LENGTH  0x08 /* 126/127 form used for a length that fits a shorter form */
#define XYWS_ST_LENGTH_MSB         0x10 /* 64-bit length with the most significant bit set */
#define XYWS_ST_BAD_CONTROL        0x20 /* control frame (opcode >= 8) with FIN=0 or length > 125 */
#define XYWS_ST_UNMASKED           0x40 /* MASK bit clear (client frames must be masked) */
#define XYWS_ST_OVERLAP            0x80 /* indexed mode: frame overlaps the next caller-supplied start;
                                           its unmask is clipped at that start */

/* ---- decode options ----------------------------------------------------- */
#define XYWS_OPT_PARSE_ONLY     0x1u /* build the frame table, leave payload bytes untouched */
#define XYWS_OPT_UNMASKED_HINT  0x2u /* stream mode: speculate on server->client (MASK=0) framing */
#define XYWS_OPT_SERIAL_SCAN    0x4u /* stream mode: one-lane serial boundary chase (debug/reference
                                        shape; exact, slow). Default is the fused tile kernel. */

/* One decoded frame. 32 bytes, naturally aligned; written to device memory. */
typedef struct xyws_frame {
  int64_t  frame_off;   /* header byte 0 relative to the batch start (< 0: header began in
                           an earlier batch and was completed from xyws_carry.hdr)        */
  int64_t  payload_off; /* payload byte 0 relative to the batch start                      */
  uint64_t payload_len; /* raw parsed length (websocket_frame_header_parser::length())    */
  uint8_t  key[4];      /* masking key, wire order (== bytes of mask_uint32_t(), :259-262) */
  uint8_t  flags;       /* websocket_flags: opcode | FIN 0x10 | HAS_MASK 0x20             */
  uint8_t  hdr_len;     /* 2..14: value parse() returns when fed from the frame start     */
  uint8_t  status;      /* XYWS_ST_* bits                                                  */
  uint8_t  reserved;
} xyws_frame;

/*
 * Decoder state carried across batch boundaries — the device-side analogue of
 * websocket_mask's returned phase `i` (websocket_frame_mask.h:14,24) and of the
 * parser's incremental npos protocol (websocket_frame_header.h:230,383-384).
 * A byte stream split at ANY point into consecutive batches decodes to the same
 * bytes and the same frames as the unsplit stream. A zero-filled carry is the
 * state at a frame boundary (a fresh parser).
 */
typedef struct xyws_carry {
  uint64_t payload_remaining; /* payload bytes of the open frame not yet seen (0 = at a boundary) */
  uint64_t phase;             /* websocket_mask phase for the next payload byte of the open frame */
  uint64_t frames_total;      /* frames whose header completed in all earlier batches             */
  uint8_t  key[4];            /* key of the open frame (wire order)                               */
  uint8_t  hdr_len;           /* bytes of an incomplete header held in hdr[] (0..13)              */
  uint8_t  hdr[14];           /* the incomplete header's bytes                                    */
  uint8_t  reserved[21];
} xyws_carry;                 /* 64 bytes */

typedef struct xyws_ctx xyws_ctx;

/* ---- library / context --------------------------------------------------- */
int         xyws_abi_version(void);
const char* xyws_strerror(int code);

/* Bind a context to HIP device `device`. One context per (thread, device). */
int xyws_ctx_create(int device, xyws_ctx** out);
int xyws_ctx_destroy(xyws_ctx* ctx);
/* Pre-size scratch for batches up to `max_batch_bytes` (and, for indexed mode
 * and frame descriptors, `max_frames` frames) so that later calls allocate
 * nothing and can be captured into a hipGraph. The per-frame tables go to the
 * streams already used on the context and to one spare: the first stream new
 * to the context may be captured at once; a second new stream needs one
 * uncaptured call first (or XYWS_ERR_CAPACITY). A stream that gets them gets
 * whatever this call and xyws_ctx_reserve_iov have reserved so far, whichever
 * call it is. Calls on larger batches grow scratch lazily. */
int xyws_ctx_reserve(xyws_ctx* ctx, uint64_t max_batch_bytes, uint64_t max_frames);
/* The staging buffer of xyws_decode_stream_iov for sequences of up to
 * `max_total_bytes` in all, in the slots of the streams already used on the
 * context and in one spare (the same streams, by the same rule, as
 * xyws_ctx_reserve's per-frame tables): with
 * xyws_ctx_reserve(ctx, max_total_bytes, ...) before it, an iov decode that
 * fits allocates nothing and can be captured into a hipGraph. */
int xyws_ctx_reserve_iov(xyws_ctx* ctx, uint64_t max_total_bytes);
/* Device-side error word of the last completed call (0 = none; its bits are
 * the DERR_* of xynet_amd/csrc/xyws_stream.h). Synchronizes the context's
 * device. */
int xyws_ctx_last_device_error(xyws_ctx* ctx, uint32_t* out);

/* ---- hot path ------------------------------------------------------------ */

/* websocket_mask (websocket_frame_mask.h:6-25) on device memory: in place,
 * dev[j] ^= key[(phase + j) % 4] for j in [0, len). *phase_out (host pointer,
 * nullable) receives phase + len, the reference's return value. Eager calls
 * claim 64 KiB tiles from a counter in the stream's scratch slot (reset by
 * the launch itself); a call captured into a graph needs no reserve and
 * leaves no state outside its launch (static tiles), so its replays may run
 * on any stream, concurrently with each other. */
int xyws_unmask(xyws_ctx* ctx, void* dev, uint64_t len, const uint8_t key[4],
                uint64_t phase, uint64_t* phase_out, void* stream);

/* websocket_mask(R&& data, uint32_t mask, size_t i) with the reference's
 * contract (websocket_frame_mask.h:14, called by websocket_recv_data at
 * example/include/common/websocket.h:131): `data` is host or device memory,
 * and the bytes are unmasked when the call returns (it synchronizes
 * `stream`). Host bytes are staged through the context's device buffer (a
 * compatibility path: two copies per call); device bytes go to xyws_unmask.
 * Not allowed during stream capture (XYWS_ERR_CAPACITY). */
int xyws_mask_bytes(xyws_ctx* ctx, void* data, uint64_t len, const uint8_t key[4],
                    uint64_t phase, uint64_t* phase_out, void* stream);
/* xyws_mask_bytes refuses device memory of another device than ctx's
 * (XYWS_ERR_INVALID; xyws_unmask takes ctx's device memory only, unchecked:
 * no pointer query on the hot path). xyws_pointer_device: *device = the HIP device whose
 * memory `p` points into, or -1 for host memory (pinned, registered or
 * pageable); the shim uses it to pick the per-device context. */
int xyws_pointer_device(const void* p, int* device);

/* Frames at caller-known offsets (ascending, non-overlapping) inside one
 * device buffer: parse each header as websocket_frame_header_parser::parse
 * does from a fresh parser, then unmask its payload in place (clipped to the
 * buffer). A header that does not fit in the buffer yields hdr_len = 0 and is
 * left untouched. `dev_frames` (nullable) receives n descriptors. */
int xyws_decode_indexed(xyws_ctx* ctx, void* dev_buf, uint64_t len,
                        const uint64_t* dev_starts, uint64_t n,
                        xyws_frame* dev_frames, uint32_t opts, void* stream);

/* Back-to-back frames in one device buffer, boundaries discovered on device:
 * the batched websocket_recv_data (websocket.h:110-134) without its caller
 * policy. Starting from `dev_carry_in` (nullable = fresh stream), every frame
 * is parsed with a fresh parser and its payload unmasked in place; a frame or
 * header cut by the batch end is continued through `dev_carry_out`
 * (nullable). Up to `cap` descriptors go to `dev_frames` (nullable); the frame
 * count (which may exceed cap) goes to `dev_nframes` (nullable). All
 * pointers except ctx are device pointers. dev_carry_in may equal
 * dev_carry_out. */
int xyws_decode_stream(xyws_ctx* ctx, void* dev_buf, uint64_t len,
                       const xyws_carry* dev_carry_in, xyws_carry* dev_carry_out,
                       xyws_frame* dev_frames, uint64_t cap, uint64_t* dev_nframes,
                       uint32_t opts, void* stream);

/* One piece of a buffer sequence: device memory. */
typedef struct xyws_iov {
  void*    base;
  uint64_t len;
} xyws_iov;
#define XYWS_IOV_MAX 64u
/* xyws_decode_stream over a buffer sequence — what one recv into a
 * multi-buffer `buffer_sequence` fills (include/xynet/buffer.h:94-110,
 * socket/impl/recv_all.h:99-121): the `niov` pieces (a HOST array of device
 * pieces, at most XYWS_IOV_MAX, any lengths and alignments, 0-length pieces
 * allowed) are ONE stream, decoded as if concatenated; every piece is
 * unmasked in place. Descriptor offsets count bytes across the pieces in
 * order (piece k starts at the sum of the earlier pieces' lengths). The
 * call takes one of three paths:
 *  - single piece: one non-empty piece is decoded as xyws_decode_stream
 *    decodes that buffer;
 *  - pieces in place: several non-empty pieces, no descriptors asked for
 *    (dev_frames null or cap 0), and every non-empty piece at least 64 MiB
 *    when the stream's previous call found frames of one size, else at least
 *    256 MiB: one decode per piece where it lies, the carry chained from
 *    piece to piece on the device;
 *  - staged: everything else. Three launches whatever niov (gather into the
 *    stream's staging buffer, one decode, scatter back); the staging buffer
 *    grows to the largest total seen (XYWS_ERR_CAPACITY under capture before
 *    it has, or before xyws_ctx_reserve_iov reserved it).
 * Every path sizes and reserves all the scratch the call needs before it
 * queues any work: an error other than XYWS_ERR_HIP means that nothing was
 * queued and the caller's buffers are untouched, so the call may be repeated.
 * (The options XYWS_OPT_IOV_PIECES and XYWS_OPT_IOV_STAGE that force the
 * second or third path are internal, for tests and measurements.)
 * XYWS_OPT_SERIAL_SCAN is refused (XYWS_ERR_INVALID). */
int xyws_decode_stream_iov(xyws_ctx* ctx, const xyws_iov* iov, uint32_t niov,
                           const xyws_carry* dev_carry_in, xyws_carry* dev_carry_out,
                           xyws_frame* dev_frames, uint64_t cap, uint64_t* dev_nframes,
                           uint32_t opts, void* stream);


/* ==== ABI 2: the rest of the frame interface ============================ */

#define XYWS_NPOS UINT64_MAX /* websocket_frame_header_parser::npos (:230) */

/* ---- websocket_frame_header_parser (websocket_frame_header.h:226-385) ---
 * The reference's incremental one-header parser. parse() feeds `len` bytes
 * (host or device memory); *consumed receives the bytes consumed in THIS call
 * up to the end of the header, or XYWS_NPOS while the header is incomplete.
 * Once a header completed, further input returns XYWS_NPOS until reset()
 * (:378-384). The bytes are parsed on the device by the stream decoder in
 * parse-only mode with a device-resident carry; parse() is synchronous on
 * `stream` (it returns the reference's answer). result() before a header
 * completed returns what the reference's state machine holds at that point
 * (:305-385): flags from the first byte, HAS_MASK and the 7-bit length from
 * the second (0 for the 126/127 forms), the extended length accumulated over
 * the bytes received, the mask bytes received so far (checked against the
 * reference's parser corpus, tests/golden/parse_corpus.json). */
typedef struct xyws_parser xyws_parser;
int xyws_parser_create(xyws_ctx* ctx, xyws_parser** out);
int xyws_parser_destroy(xyws_parser* p);
int xyws_parser_reset(xyws_parser* p);
int xyws_parser_parse(xyws_parser* p, const void* data, uint64_t len, uint64_t* consumed, void* stream);
int xyws_parser_result(const xyws_parser* p, uint8_t* flags, uint8_t key[4], uint64_t* length);

/* ---- header build (detail::websocket_frame_header_builder, :136-175) ----
 * One header into out[14] (host memory, no device work); returns its length
 * H. With XYWS_FLAG_HAS_MASK the 4 key bytes are written only when `key` is
 * non-null, as the reference builder does (:168-173); with key == NULL they
 * are zero, which is what class websocket_frame_header's masked constructors
 * produce (:183-202). */
uint64_t xyws_header_build(uint8_t flags, const uint8_t* key, uint64_t len, uint8_t out[14]);

/* ---- batched encode on the device (echo replies, client-role frames) ----
 * For every frame i < n_eff (n_eff = min(n, *dev_n) when dev_n is given) of
 * a decoded frame table, writes a reply frame = header(flags_i, len_i) +
 * payload bytes dev_src[payload_off .. +payload_len) into dev_out, replies
 * back to back in frame order (the iovec pair echo_once sends, as one
 * buffer). flags_i = `flags`, or with XYWS_ENC_FRAME_OPCODE the frame's own
 * opcode and FIN (a ping answered as a pong) plus `flags`' HAS_MASK bit.
 * With HAS_MASK and dev_keys (4 bytes per frame, wire order) the header
 * carries key i and the payload is masked with it (client role); with
 * HAS_MASK and dev_keys == NULL the key bytes are zero (the reference
 * class's form) and the payload is copied unchanged. dev_verdicts (nullable,
 * from xyws_classify_frames) with `action_mask` (bit 1<<action) selects which
 * frames get a reply (others: none). dev_offsets (nullable) receives n_eff+1
 * reply offsets; *dev_out_len (nullable) the total reply bytes. Bytes past
 * out_cap are not written (compare *dev_out_len with out_cap); payload bytes
 * past src_len read as zero and set DERR_SRC_OOB (0x100) in the device error
 * word. */
#define XYWS_ENC_FRAME_OPCODE 0x1u
typedef struct xyws_verdict xyws_verdict;
int xyws_encode_frames(xyws_ctx* ctx, const void* dev_src, uint64_t src_len,
                       const xyws_frame* dev_frames, uint64_t n, const uint64_t* dev_n,
                       uint8_t flags, uint32_t enc_opts, const uint8_t* dev_keys,
                       const xyws_verdict* dev_verdicts, uint32_t action_mask,
                       void* dev_out, uint64_t out_cap, uint64_t* dev_offsets,
                       uint64_t* dev_out_len, void* stream);

/* ---- close policy per frame (websocket_check_parser_result) -------------
 * websocket.h:81-108 checks, in order: close frame -> 1000, FIN=0 -> 1003,
 * unmasked -> 1008, length > max -> 1009. Here without its opcode bug (the
 * bit-3 test `flags & WS_OP_CLOSE` there also closes on ping and pong):
 * pings and pongs are actions of their own. Policy bits relax or tighten the
 * reference's checks. *dev_first_close (nullable) receives the index of the
 * first frame with a close code, or UINT64_MAX. */
#define XYWS_ACT_DATA   0 /* text/binary/continuation frame to deliver */
#define XYWS_ACT_PING   1 /* answer with a pong carrying the same payload */
#define XYWS_ACT_PONG   2 /* unsolicited or answering pong: nothing to do */
#define XYWS_ACT_CLOSE  3 /* the connection closes with close_code */
#define XYWS_POL_FRAGMENTS  0x1u /* accept FIN=0 data frames (reassembly) instead of closing 1003 */
#define XYWS_POL_UNMASKED   0x2u /* accept unmasked frames instead of closing 1008 */
#define XYWS_POL_STRICT     0x4u /* RFC 6455 protocol errors (RSV, reserved opcode, fragmented or
                                    >125-byte control frame) close 1002 (the reference accepts them) */
#define XYWS_POL_REFERENCE  0x8u /* the reference's own close test, bug included: `flags & WS_OP_CLOSE`
                                    (websocket.h:87) is bit 3 of the opcode, so ping, pong and opcodes
                                    0xB-0xF close 1000 like a close frame (echo_once answers nothing else) */
struct xyws_verdict {
  uint16_t close_code; /* 0, or the code the connection closes with */
  uint16_t peer_code;  /* close frames: the peer's status code (1005 if none) */
  uint8_t  action;     /* XYWS_ACT_* */
  uint8_t  reserved[3];
};
int xyws_classify_frames(xyws_ctx* ctx, const void* dev_src, uint64_t src_len,
                         const xyws_frame* dev_frames, uint64_t n, const uint64_t* dev_n,
                         uint64_t max_payload, uint32_t policy, xyws_verdict* dev_verdicts,
                         uint64_t* dev_first_close, void* stream);

/* ---- message reassembly (FIN=0 chains) + UTF-8 validation ---------------
 * A message is a text/binary frame followed by continuation frames up to the
 * first one with FIN (control frames may sit between fragments and are not
 * part of it). Every message's payload is gathered into dev_out back to back
 * (frame payloads must be complete in dev_src: decoded, unmasked); its
 * record goes to dev_msgs[m] in order; *dev_nmsgs receives the count. With
 * XYWS_REASM_UTF8 every text message is validated (RFC 3629: no overlongs,
 * surrogates or code points above U+10FFFF). A continuation outside a
 * message is dropped and reported with XYWS_MSG_ORPHANS on the next message
 * (DERR_ORPHANS (0x200) in the device error word if none follows). */
#define XYWS_REASM_UTF8 0x1u
#define XYWS_MSG_COMPLETE   0x1u /* the FIN fragment is in this batch */
#define XYWS_MSG_UTF8_BAD   0x2u /* text message: invalid UTF-8 (a sequence cut by the end of an
                                    incomplete message is not counted) */
#define XYWS_MSG_INTERRUPTED 0x4u /* a new text/binary frame started before the FIN fragment */
#define XYWS_MSG_TRUNCATED  0x8u /* the payload did not fit in out_cap */
#define XYWS_MSG_ORPHANS    0x10u /* continuation frames without a message preceded this one */
typedef struct xyws_message {
  uint64_t first_frame; /* index of the text/binary frame that starts it */
  uint64_t nframes;     /* its data frames */
  uint64_t out_off;     /* its payload in dev_out */
  uint64_t length;      /* total payload bytes */
  uint32_t status;      /* XYWS_MSG_* */
  uint8_t  opcode;      /* XYWS_FLAG_OP_TEXT or XYWS_FLAG_OP_BINARY */
  uint8_t  reserved[3];
} xyws_message;         /* 40 bytes */
int xyws_reassemble(xyws_ctx* ctx, const void* dev_src, uint64_t src_len,
                    const xyws_frame* dev_frames, uint64_t n, const uint64_t* dev_n, uint32_t opts,
                    void* dev_out, uint64_t out_cap, xyws_message* dev_msgs, uint64_t msg_cap,
                    uint64_t* dev_nmsgs, void* stream);

/* ---- message reassembly across batch boundaries --------------------------
 * xyws_reassemble for a stream cut at any point into batches: the frame table
 * is the one xyws_decode_stream wrote for this same dev_src (unmasked, every
 * frame of the batch, in order; frame_off < 0 allowed for the first frame),
 * and xyws_msg_carry continues the open message, the frame cut by the batch
 * end, pending orphans and a cut UTF-8 sequence into the next call. Both
 * carries are device pointers; dev_mc_in NULL = a fresh stream; dev_mc_in may
 * equal dev_mc_out. Asynchronous, no host read of device state; scratch and
 * the capture rule are xyws_reassemble's.
 *
 * Bytes. The first min(mc_in.frame_remaining, src_len) bytes of dev_src are
 * the rest of the frame the previous batch end cut: they join the open
 * message when frame_member is set and are skipped otherwise. A frame's
 * payload contributes the bytes that lie in this batch,
 * min(payload_len, src_len - payload_off) (only the last frame can be
 * clipped; the missing part becomes mc_out.frame_remaining). Clipping never
 * sets DERR_SRC_OOB. Everything goes to dev_out back to back in stream order.
 *
 * Records. With a message open in mc_in, record 0 is always its continuation
 * (also with no bytes and no frames): XYWS_MSG_CONTINUED, first_frame =
 * XYWS_NPOS, nframes = its data frames with a descriptor in this table,
 * length = the bytes this call delivered, out_off 0, opcode and the sticky
 * bits (UTF8_BAD, UNCHECKED) from the carry. Every other record is
 * xyws_reassemble's for this table (first_frame an index into it). COMPLETE
 * is reported by the call that delivers the message's LAST BYTE: when the FIN
 * fragment's descriptor is in the table but its payload is cut, the message
 * stays open in mc_out (status has XYWS_MSG_COMPLETE there: "closing") and
 * the call that delivers the last of frame_remaining emits CONTINUED|COMPLETE.
 * INTERRUPTED: a text/binary frame started before the FIN. A message open at
 * the batch end has neither bit and goes to mc_out. A continuation is an
 * orphan only when no message is open (the carry counted); orphans with no
 * message after them are carried (status ORPHANS with opcode 0) and flagged
 * on the next message start, in whichever call; DERR_ORPHANS is never raised.
 * TRUNCATED and msg_cap act per call. A text message becomes UNCHECKED for the
 * rest of its life (sticky; later calls neither validate it nor keep a UTF-8
 * tail) when a call truncated its bytes by out_cap, could not store its
 * record (msg_cap), or ran without validation (no XYWS_REASM_UTF8, or out_cap
 * or msg_cap 0). The structural carry fields (opcode, length, nframes,
 * first_frame, frame_remaining, frame_member, frames_seen, pending orphans)
 * are exact whatever out_cap and msg_cap.
 *
 * UTF-8. A lead byte in the last 3 bytes of a message that stays open, whose
 * sequence runs past the batch end, is not judged in that call: the bytes
 * from the earliest such lead on go to mc_out.utf8 (1..3; a short batch may
 * extend them), and the sequence is judged whole (second-byte rules of E0, ED,
 * F0, F4 included) by the call that supplies its last byte; if the message
 * completes first it is invalid. UTF8_BAD is sticky through the carry. So the
 * record that completes a message has UTF8_BAD exactly when xyws_reassemble
 * on the unsplit stream sets it. */
#define XYWS_MSG_CONTINUED 0x20u /* stream mode: the message began in an earlier call; this record holds
                                    only the part delivered by this call */
#define XYWS_MSG_UNCHECKED 0x40u /* stream mode: text message whose UTF-8 validation was abandoned in an
                                    earlier call (see above); UTF8_BAD, if set, was found before that */
typedef struct xyws_msg_carry {  /* 64 bytes; all zero = a fresh stream */
  uint64_t length;          /* payload bytes of the open message delivered by all calls so far */
  uint64_t nframes;         /* its data frames whose descriptor was in a table so far */
  uint64_t first_frame;     /* stream-wide index of its first frame (frames_seen at that call + index) */
  uint64_t frame_remaining; /* payload bytes of the frame cut by the last batch end, still to come */
  uint64_t frames_seen;     /* sum of n_eff over all calls so far */
  uint32_t status;          /* sticky bits ORed into the open message's next record (UTF8_BAD, UNCHECKED),
                               and XYWS_MSG_COMPLETE while it is closing (FIN fragment seen, bytes to
                               come); with no message open: XYWS_MSG_ORPHANS = orphans seen, no message
                               since */
  uint8_t  opcode;          /* 0 = no message open, else XYWS_FLAG_OP_TEXT / _BINARY */
  uint8_t  frame_member;    /* 1: the frame_remaining bytes belong to the open message; 0: skip them
                               (control frame or orphan continuation) */
  uint8_t  utf8_len;        /* 0..3 bytes of a UTF-8 sequence cut by the last batch end ... */
  uint8_t  utf8[3];         /* ... from its lead byte on */
  uint8_t  reserved[14];    /* zero */
} xyws_msg_carry;
int xyws_reassemble_stream(xyws_ctx* ctx, const void* dev_src, uint64_t src_len,
                           const xyws_frame* dev_frames, uint64_t n, const uint64_t* dev_n, uint32_t opts,
                           const xyws_msg_carry* dev_mc_in, xyws_msg_carry* dev_mc_out,
                           void* dev_out, uint64_t out_cap, xyws_message* dev_msgs, uint64_t msg_cap,
                           uint64_t* dev_nmsgs, void* stream);

/* ---- recv arenas: the io_uring side (recv_all.h:86-121, io_service.h:362-381)
 * One arena per connection: a receive area in pinned host memory (allocated
 * here, or the caller's buffer registered with hipHostRegister, e.g. the
 * memory an io_uring registered-buffer ring hands to recv), a device mirror,
 * a device-resident carry and up to XYWS_ARENA_SLOTS submissions in flight on
 * one of the context's arena streams (arenas share 8 streams round robin, so
 * any number of connections binds at most 8 scratch slots; an arena's
 * submissions stay in order). xyws_arena_submit(offset, len) enqueues
 * H2D -> xyws_decode_stream (carry chained across submissions, so a frame cut
 * by a recv boundary decodes as if unsplit) -> D2H of the unmasked bytes back
 * into the same host range (in place, like websocket_mask) and of the frame
 * table and count, then a host callback that marks the submission complete
 * and writes 1 to the arena's eventfd (when one is given): the ring keeps a
 * poll_add on that fd exactly as io_service does for its remote-queue eventfd
 * and never blocks on the GPU. xyws_arena_poll() returns XYWS_ERR_AGAIN until
 * the submission completed. Submissions complete in order. A submission's
 * results stay valid until its slot is reused, which happens only after
 * poll() or wait() returned them: submit() returns XYWS_ERR_AGAIN while
 * XYWS_ARENA_SLOTS submissions are in flight or unclaimed. wait() blocks on
 * that submission's own completion event, not on the shared stream (other
 * connections' later work is not waited for). Arenas that share a stream
 * share its scratch slot, so the decoder choice one arena's batches steer
 * (which decoder, which geometry: speed only, never bytes) applies to the
 * next batch of any arena on that stream. */
#define XYWS_ARENA_SLOTS 8
/* A submit that fails before anything was enqueued leaves the arena as it
 * was; one that fails later (the decode or a copy back could not be
 * enqueued) leaves it failed: the device carry may have moved past bytes no
 * result reports, so every later submit returns XYWS_ERR_HIP (destroy it). */
typedef struct xyws_arena xyws_arena;
typedef struct xyws_arena_result {
  uint64_t seq;              /* the submission */
  uint64_t offset, len;      /* its host range (now unmasked in place) */
  uint64_t nframes;          /* frames whose header completed in it */
  const xyws_frame* frames;  /* min(nframes, max_frames) descriptors, pinned host memory, offsets
                                relative to `offset`; valid until the slot is reused */
  xyws_carry carry;          /* the connection's carry after it */
} xyws_arena_result;
/* host == NULL: allocate `bytes` of pinned memory; else register the caller's
 * host range (unregistered at destroy). eventfd < 0: no notification. */
int xyws_arena_create(xyws_ctx* ctx, void* host, uint64_t bytes, uint64_t max_frames, int eventfd,
                      xyws_arena** out);
int xyws_arena_destroy(xyws_arena* a);
void* xyws_arena_host(xyws_arena* a);
int xyws_arena_submit(xyws_arena* a, uint64_t offset, uint64_t len, uint32_t opts, uint64_t* seq);
int xyws_arena_poll(xyws_arena* a, uint64_t seq, xyws_arena_result* out);
int xyws_arena_wait(xyws_arena* a, uint64_t seq, xyws_arena_result* out);
/* The completion notifier on its own (no device): what the arena's host
 * callback runs. Exposed so the eventfd handshake can be exercised on a host
 * without a GPU. */
typedef struct xyws_notifier xyws_notifier;
int xyws_notifier_create(int eventfd, xyws_notifier** out);
int xyws_notifier_destroy(xyws_notifier* n);
int xyws_notifier_signal(xyws_notifier* n, uint64_t seq); /* marks seq complete, writes the fd */
uint64_t xyws_notifier_completed(const xyws_notifier* n); /* highest completed seq + 1 */
/* xyws_notifier_signal(n, seq) run by `stream` itself, once it has passed
 * everything enqueued before: a hipLaunchHostFunc callback, so that the ring
 * learns through the eventfd that a sweep's outbox (xyws_outbox_streams) is
 * ready as it does for an arena submission. Not for a capturing stream. The
 * callback's block lives in the notifier, in a ring of 64: XYWS_ERR_AGAIN when
 * the callback that last used this one's slot has not run yet. The notifier is
 * destroyed only after every callback ran. */
int xyws_notifier_enqueue(xyws_notifier* n, uint64_t seq, void* stream);

/* ---- one batch across several devices -----------------
 * Frames are independent, so a batch of back-to-back frames splits across
 * devices at frame boundaries with no exchange between them. xyws_shard_plan
 * cuts `len` bytes of host memory (what a recv buffer_sequence holds,
 * buffer.h:94-224 / recv_all.h:99-121 of the reference) into n_shards
 * contiguous ranges bounds[k] .. bounds[k+1] (n_shards + 1 entries, bounds[0]
 * = 0, bounds[n_shards] = len) balanced by bytes: bounds[k] is the frame
 * start nearest to k * len / n_shards (each shard is within one frame of
 * len / n_shards). Shard 0 continues from `carry_in` (nullable = a fresh
 * stream); every other shard starts at a frame boundary, so it decodes on its
 * own device with a fresh carry (xyws_decode_stream, dev_carry_in = NULL) to
 * exactly the bytes and frames of the unsplit decode; only the last shard can
 * end inside a frame (its carry out continues the stream). The headers are
 * walked on the host (one header read per frame, parsed as
 * websocket_frame_header_parser::parse, websocket_frame_header.h:305-385):
 * a planner, not a decode — no payload byte is touched. A shard may be empty
 * when one frame is larger than len / n_shards. */
int xyws_shard_plan(const void* host_batch, uint64_t len, const xyws_carry* carry_in, uint32_t n_shards,
                    uint64_t* bounds);
/* The same from a frame table in host memory (frame_off ascending: e.g. the
 * descriptors of a parse-only decode, or the table a generator or a framing
 * layer already holds): the candidate boundaries are the frame_off >= 0
 * values (a negative frame_off, a header carried in, is not one) and len. */
int xyws_shard_plan_frames(const xyws_frame* frames, uint64_t n, uint64_t len, uint32_t n_shards,
                           uint64_t* bounds);

/* ---- many connections, one call ------------------------------------------
 * What an io_uring service holds after one sweep of its completion queue: a
 * few hundred bytes to a few KiB for each of hundreds or thousands of
 * connections, every connection with a parser state of its own. One launch
 * decodes them all, one wave per connection, thousands side by side.
 *
 *  - Entry i is decoded exactly as xyws_decode_stream(ctx, buf_i, len_i,
 *    carry_i, carry_i, frames_i, cap_i, &dev_nframes[i], opts, stream) would
 *    decode it: the bytes, the descriptors with their status bits, the count
 *    (which may exceed cap_i), the carry and its frames_total.
 *  - Buffers may have any alignment and any length. Bytes outside
 *    [buf_i, buf_i + len_i) are never written; two connections' buffers may
 *    share a 16-byte line, as adjacent ranges of one receive slab do.
 *  - dev_conns is device memory. The entries' buffers must not overlap, and a
 *    carry must not appear in two entries of one call.
 *  - n == 0 returns XYWS_OK and launches nothing.
 *  - opts may be XYWS_OPT_PARSE_ONLY or XYWS_OPT_UNMASKED_HINT (accepted and
 *    ignored: nothing is speculated here); every other bit is
 *    XYWS_ERR_INVALID. A null ctx, or null dev_conns with n > 0, is
 *    XYWS_ERR_INVALID.
 *  - The call is one launch. It uses no context scratch, binds no scratch
 *    slot of the stream and reads or writes no policy word: it needs no
 *    reserve and can be captured into a hipGraph at once, calls on different
 *    streams run concurrently, and the stream's history for
 *    xyws_decode_stream stays as it was.
 *  - Meant for many connections of up to about 1 MiB each. It is correct for
 *    any length, but one wave walks a connection from end to end: one very
 *    long stream belongs to xyws_decode_stream. */
/* One connection's share of a multi-connection decode. 64 bytes. */
typedef struct xyws_conn {
  void*       buf;         /* device: the bytes this connection received since its last call */
  uint64_t    len;         /* 0 allowed: the connection is left as it is, its count is 0 */
  xyws_carry* carry;       /* device; read, then written (in == out). NULL: a fresh stream, no state kept */
  xyws_frame* frames;      /* device, nullable: up to cap descriptors, offsets relative to buf */
  uint64_t    cap;
  uint64_t    reserved[3]; /* zero */
} xyws_conn;
int xyws_decode_streams(xyws_ctx* ctx, const xyws_conn* dev_conns, uint64_t n,
                        uint64_t* dev_nframes /* n entries, nullable */,
                        uint32_t opts, void* stream);

/* ---- many connections, one reply call -------------------------------------
 * The other half of the reference's per-connection loop, for every connection
 * of an xyws_decode_streams call at once: websocket_check_parser_result,
 * echo_once and websocket_send_close (example/include/common/websocket.h:70-108,
 * example/websocket/websocket_echo.cpp:18-27). dev_conns and dev_nframes are
 * the table and the counts the xyws_decode_streams call just before it used
 * and wrote (of dev_conns[i] only buf, len, frames and cap are read; buf holds
 * the decoded bytes); dev_replies[i] names connection i's send buffer, its
 * reply carry and (nullable) a row of verdicts. Server role: replies are
 * unmasked. Per connection, with t = dev_nframes[i] and the carry rc:
 *
 *  1. Overflow. rc.status has XYWS_RPL_OVERFLOW, or t > cap, or frames is
 *     NULL while t > 0: nothing is written to out or verdicts, the result is
 *     reply_len 0 with status OVERFLOW, and rc.status keeps OVERFLOW (the
 *     table no longer covers the stream: the caller closes the connection).
 *  2. Closed. rc.close_code != 0: nothing is written; the result is reply_len
 *     0, status CLOSED, close_code from the carry, first_close XYWS_NPOS. The
 *     carry is unchanged.
 *  3. Continued frame. k = min(rc.frame_remaining, len); with rc.echoing the
 *     bytes buf[0..k) go to the reply first. frame_remaining -= k.
 *  4. Verdict j is xyws_classify_frames' for this table with src = buf,
 *     src_len = len, max_payload and policy; it is stored to verdicts[j] when a
 *     row is given. c = the first j with a close code, or t.
 *  5. Every frame j < c with (action_mask >> action_j) & 1 is answered:
 *     header(reply_flags_j, payload_len_j), built as xyws_encode_frames builds
 *     it without keys (XYWS_ENC_FRAME_OPCODE: the frame's own opcode and FIN, a
 *     ping answered as a pong), then the payload bytes that lie in this batch:
 *     inb = min(payload_len, len - payload_off), 0 if payload_off >= len (only
 *     the last frame can be clipped). Nothing outside [buf, buf + len) is
 *     read, whatever the table says (whole 16-byte lines that hold one of its
 *     bytes are loaded). After frame j: frame_remaining = payload_len - inb,
 *     echoing = answered.
 *  6. Close. If c < t the reference's close frame 0x88 0x02 hi lo with
 *     verdict c's close_code ends the reply; rc.close_code = that code,
 *     first_close = c, status CLOSED. Frames after c get verdicts, no reply.
 *     The close is decided on the header alone: a cut frame that is too long
 *     closes 1009 in the call that sees its header.
 *  7. frames_seen += t, replies_total += answered.
 *  8. Reply bytes at positions >= out_cap are not written; reply_len is the
 *     full length, XYWS_RPL_TRUNCATED is set when reply_len > out_cap, and the
 *     carry is exact whatever out_cap. No byte outside
 *     [out, out + min(reply_len, out_cap)) is written: neighbouring
 *     connections' out ranges may share a 16-byte line, as in a send slab.
 *  9. out_cap >= len + 13 always suffices for a table xyws_decode_streams
 *     wrote: a frame whose header bytes lie in this batch has a reply header
 *     no longer than them (2, 4 or 10 bytes against 2..14 received, the reply
 *     length form being the minimal one), so it adds nothing; only the one
 *     frame whose header was carried in (frame_off < 0) can have a reply
 *     header longer than its header bytes in this batch, by at most 10 - 1
 *     bytes (at least one header byte arrives with the batch that completes
 *     it); the close frame adds 4: len + 9 + 4.
 *
 * So for a stream cut at any points into calls, the concatenation of the
 * calls' replies equals xyws_encode_frames of the unsplit stream's frames
 * before its first close (verdicts of xyws_classify_frames), followed by the
 * close frame if any; while the connection is open rc.frame_remaining equals
 * xyws_carry.payload_remaining after every call.
 *
 * Like xyws_decode_streams the call is one launch (one wave per connection),
 * uses no context scratch, no scratch slot and no policy word, reads no
 * device state on the host, needs no reserve, can be captured into a hipGraph
 * at once and runs concurrently on different streams. n == 0 returns XYWS_OK
 * and launches nothing. XYWS_ERR_INVALID: a null ctx; null dev_conns,
 * dev_nframes or dev_replies with n > 0; flags with XYWS_FLAG_HAS_MASK;
 * enc_opts bits other than XYWS_ENC_FRAME_OPCODE; unknown policy bits;
 * action_mask bits above 1 << XYWS_ACT_CLOSE. The out ranges must not overlap
 * each other or a recv buffer; a reply carry must not appear twice in a call. */
typedef struct xyws_reply_carry {   /* 32 bytes; all zero = a fresh connection */
  uint64_t frame_remaining; /* payload bytes of the frame cut by the last batch end, still to come */
  uint64_t frames_seen;     /* sum of the table sizes of all calls so far */
  uint64_t replies_total;   /* frames answered so far */
  uint16_t close_code;      /* != 0: closed with this code (sticky; later calls write nothing) */
  uint8_t  echoing;         /* 1: the frame_remaining bytes belong to a reply already begun */
  uint8_t  status;          /* XYWS_RPL_OVERFLOW, sticky */
  uint8_t  reserved[4];     /* zero */
} xyws_reply_carry;

typedef struct xyws_reply_conn {    /* 32 bytes; entry i goes with dev_conns[i] */
  void*             out;      /* device: this connection's send buffer */
  uint64_t          out_cap;
  xyws_reply_carry* rc;       /* device; read, then written. NULL: fresh, no state kept */
  xyws_verdict*     verdicts; /* device, nullable: one per frame of its table */
} xyws_reply_conn;

typedef struct xyws_reply_result {  /* 32 bytes */
  uint64_t reply_len;   /* bytes of the reply (may exceed out_cap: then TRUNCATED) */
  uint64_t first_close; /* index in this call's table of the frame that closed it, or XYWS_NPOS */
  uint32_t answered;    /* frames whose reply header this call wrote */
  uint16_t close_code;  /* the carry's after this call */
  uint16_t status;      /* XYWS_RPL_* */
  uint64_t reserved;
} xyws_reply_result;
#define XYWS_RPL_TRUNCATED 0x1u
#define XYWS_RPL_CLOSED    0x2u  /* closed by this call or an earlier one */
#define XYWS_RPL_OVERFLOW  0x4u

int xyws_reply_streams(xyws_ctx* ctx, const xyws_conn* dev_conns, const uint64_t* dev_nframes,
                       const xyws_reply_conn* dev_replies, uint64_t n,
                       uint64_t max_payload, uint32_t policy, uint8_t flags, uint32_t enc_opts,
                       uint32_t action_mask, xyws_reply_result* dev_results /* n, nullable */,
                       void* stream);

/* ---- many connections, one reassembly call --------------------------------
 * The message side of the same sweep: what the reference's chat server does
 * with every connection's frames (example/websocket/websocket_chat.cpp:177-200,
 * one text message per connection handed on to a room), for every connection
 * of an xyws_decode_streams call at once. dev_conns and dev_nframes are the
 * table and the counts of the xyws_decode_streams call just before it (of
 * dev_conns[i] only buf, len, frames and cap are read); dev_reasm[i] names
 * connection i's message buffer, its message carry and its record row. The
 * call does not write buf: it may run before or after xyws_reply_streams for
 * the same sweep. Per connection, with t = dev_nframes[i]:
 *
 *  1. Overflow. mc->status has XYWS_MSG_OVERFLOW, or t > cap, or frames is
 *     NULL while t > 0: nothing is written to out or msgs, the result is
 *     out_len 0, nmsgs 0, status OVERFLOW, and the carry is left as it was
 *     except that status gains XYWS_MSG_OVERFLOW (the table no longer covers
 *     the stream: the caller closes the connection). A carry with this bit
 *     belongs to this call only: xyws_reassemble_stream does not know it.
 *  2. Otherwise the entry is processed exactly as
 *     xyws_reassemble_stream(ctx, buf, len, frames, t, NULL, opts, mc, mc, out,
 *     out_cap, msgs, msg_cap, &nmsgs, stream) processes it: the bytes
 *     out[0 .. min(out_len, out_cap)), the first min(nmsgs, msg_cap) records,
 *     the count and all 64 carry bytes. Everything said there holds here per
 *     connection (the continued frame, CONTINUED, closing / COMPLETE,
 *     INTERRUPTED, carried orphans, TRUNCATED, UNCHECKED, the cut UTF-8 tail,
 *     the structural carry exact whatever the caps); len == 0 with a message
 *     open still emits the empty CONTINUED record. out_cap >= len and
 *     msg_cap >= t + 1 always suffice.
 *  3. Nothing outside [buf, buf + len) is read, whatever the table says (whole
 *     16-byte lines that hold one of its bytes are loaded); a payload_off
 *     outside [0, len) contributes no bytes. No byte outside
 *     [out, out + min(out_len, out_cap)) and no record beyond
 *     min(nmsgs, msg_cap) is written: neighbouring connections' out ranges may
 *     share a 16-byte line, as in a slab. The out ranges must not overlap each
 *     other or a recv buffer; a carry must not appear twice in a call.
 *
 * Like its two siblings the call is one launch (one wave per connection), uses
 * no context scratch, no scratch slot and no policy word, never touches the
 * device error word, reads no device state on the host, needs no reserve, can
 * be captured into a hipGraph at once and runs concurrently on different
 * streams. n == 0 returns XYWS_OK and launches nothing. XYWS_ERR_INVALID: a
 * null ctx; null dev_conns, dev_nframes or dev_reasm with n > 0; opts bits
 * other than XYWS_REASM_UTF8. */
typedef struct xyws_reasm_conn {   /* 64 bytes; entry i goes with dev_conns[i] */
  void*           out;      /* device: this connection's message bytes; NULL = out_cap 0 */
  uint64_t        out_cap;
  xyws_msg_carry* mc;       /* device; read, then written. NULL: fresh, no state kept */
  xyws_message*   msgs;     /* device, nullable (then msg_cap counts as 0) */
  uint64_t        msg_cap;
  uint64_t        reserved[3]; /* zero */
} xyws_reasm_conn;

typedef struct xyws_reasm_result { /* 32 bytes */
  uint64_t out_len;   /* message bytes this call delivered (may exceed out_cap) */
  uint64_t nmsgs;     /* records of this call (may exceed msg_cap) */
  uint32_t completed; /* stored records with XYWS_MSG_COMPLETE */
  uint32_t status;    /* XYWS_RSM_* */
  uint64_t reserved;
} xyws_reasm_result;
#define XYWS_RSM_TRUNCATED 0x1u  /* out_len > out_cap */
#define XYWS_RSM_MSG_CAP   0x2u  /* nmsgs > msg_cap */
#define XYWS_RSM_OVERFLOW  0x4u
#define XYWS_RSM_OPEN      0x8u  /* a message is open in the carry after this call */
#define XYWS_RSM_UTF8_BAD  0x10u /* a stored record of this call has XYWS_MSG_UTF8_BAD */
#define XYWS_MSG_OVERFLOW  0x80u /* xyws_msg_carry.status, this call only: sticky */

int xyws_reassemble_streams(xyws_ctx* ctx, const xyws_conn* dev_conns, const uint64_t* dev_nframes,
                            const xyws_reasm_conn* dev_reasm, uint64_t n, uint32_t opts,
                            xyws_reasm_result* dev_results /* n, nullable */, void* stream);

/* ---- many connections, one broadcast call ---------------------------------
 * The room of the same chat server: chat_room::deliver hands each message to
 * every participant, the sender included, and each chat_session::writer sends
 * websocket_frame_header{FIN | TEXT, size} + (message head + payload)
 * (example/websocket/websocket_chat.cpp:89-101, 148-175). Here every room's
 * messages of one sweep are framed once into the room's wire, and the wire is
 * appended to every member's send range behind its reply: decode, reassemble,
 * reply, broadcast, with no host read of device state between the calls.
 * Server role: the frames are unmasked.
 *
 *  1. Inputs. dev_reasm is the table the xyws_reassemble_streams call of this
 *     sweep used, dev_reasm_results the rows that call wrote; both are
 *     required. Of dev_reasm[i] only out, out_cap, msgs and msg_cap are read
 *     (a NULL out counts as out_cap 0). With s_i = min(nmsgs_i, msg_cap_i) (0
 *     for a null msgs), connection i's stored records are msgs[0 .. s_i).
 *     dev_bconns[i] goes with dev_reasm[i]: the connection's message head, its
 *     send buffer, its row of this sweep's xyws_reply_streams results
 *     (nullable) and its room.
 *  2. Deliverable record. Record r of connection i is deliverable when all of
 *     these hold:
 *       - its status has XYWS_MSG_COMPLETE and none of CONTINUED, TRUNCATED,
 *         UTF8_BAD: a whole message delivered by this sweep. A message that
 *         spans sweeps counts as skipped here; xyws_hold_streams (below),
 *         called before this call, hands it over as such a whole record;
 *       - out_off + length <= out_cap_i: nothing outside [out, out + out_cap)
 *         is ever read, whatever a record says (whole 16-byte lines that hold
 *         one of its bytes are loaded);
 *       - the reassembly row has no XYWS_RSM_OVERFLOW;
 *       - when reply is given: its status has no XYWS_RPL_OVERFLOW; with
 *         c = first_close != XYWS_NPOS the record's first_frame < c (messages
 *         begun before the close frame); with status CLOSED and first_close ==
 *         XYWS_NPOS (closed by an earlier sweep) no record is deliverable.
 *     Known approximation: a message whose FIN fragment follows the close
 *     frame within the same sweep, its first frame lying before it, is
 *     delivered (the peer violated the protocol).
 *  3. The room's wire. Its valid members in members[] order, each member's
 *     deliverable records in record order: for each the wire gets
 *     header(f, head_len_i + length) | head_i | the message bytes, the header
 *     built as xyws_encode_frames builds it without keys (the minimal length
 *     form: 2, 4 or 10 bytes), f = flags, or with XYWS_ENC_FRAME_OPCODE flags
 *     with its opcode replaced by the record's. That is byte for byte what each
 *     chat_session::writer sends for each message, in one fixed order. Wire
 *     bytes at positions >= wire_cap are not written; wire_len, nmsgs and
 *     skipped are exact whatever wire_cap. No byte outside
 *     [wire, wire + min(wire_len, wire_cap)) is written.
 *  4. Fan-out. Connection i with room r is a receiver unless reply is given
 *     and has CLOSED or OVERFLOW: nothing follows a close frame.
 *     base = reply ? reply->reply_len : 0. A receiver gets wire_r[0 .. w),
 *     w = min(wire_len_r, wire_cap_r), at out + base; positions >= out_cap are
 *     not written; bcast_len = w, send_len = base + w, XYWS_BC_TRUNCATED is set
 *     when send_len > out_cap. A non-receiver gets bcast_len 0, send_len =
 *     base, NOT_RECEIVER; a connection with no room (XYWS_ROOM_NONE, or a room
 *     >= n_rooms) bcast_len 0, send_len = base, NO_ROOM. No byte outside
 *     [out + min(base, out_cap), out + min(send_len, out_cap)) is written:
 *     neighbouring connections' ranges may share a 16-byte line, as in a send
 *     slab, and out, wire, head and the message buffers may have any alignment.
 *  5. The caller's duties. Out ranges, wires and message buffers must not
 *     overlap; a connection must be a member of at most one room;
 *     dev_bconns[i].room must name the room that lists i. When the caller
 *     breaks these the results are unspecified; the call still touches no
 *     memory outside the ranges the tables name. A members[] entry >= n is
 *     ignored, never dereferenced, and reported (XYWS_ROOM_BAD_MEMBER).
 *  6. Sizing. A frame is its message's length_ir plus head_len_i plus a header
 *     of at most 10 bytes, and a member's deliverable messages are disjoint
 *     parts of its out_len_i message bytes, at most s_i of them, so
 *     wire_cap >= sum over members (out_len_i + s_i * (10 + head_len_i)) always
 *     suffices. The reply is at most len_i + 13 bytes (xyws_reply_streams, 9.)
 *     and the wire appended at most wire_cap_r, so
 *     out_cap >= (len_i + 13) + wire_cap_r always suffices for a send buffer.
 *  7. Properties. At most two launches on `stream`: the wire build (one
 *     workgroup per room; omitted when n_rooms == 0), then the fan-out;
 *     dev_room_results is the hand-over between them, which is why it is
 *     required. Like its siblings the call uses no context scratch, no scratch
 *     slot and no policy word, never touches the device error word, reads no
 *     device state on the host, needs no reserve, can be captured into a
 *     hipGraph at once and runs concurrently on different streams. n == 0
 *     returns XYWS_OK and launches nothing. XYWS_ERR_INVALID: a null ctx; null
 *     dev_reasm, dev_reasm_results or dev_bconns with n > 0; null dev_rooms or
 *     dev_room_results with n_rooms > 0; n >= UINT32_MAX; flags with
 *     XYWS_FLAG_HAS_MASK; enc_opts bits other than XYWS_ENC_FRAME_OPCODE. Every
 *     refusal is decided on the arguments alone, before the context is used. */
#define XYWS_ROOM_NONE UINT32_MAX

typedef struct xyws_room {            /* 32 bytes */
  const uint32_t* members;   /* device: indices into the connection tables, in delivery order */
  uint64_t        n_members;
  void*           wire;      /* device, nullable (then wire_cap counts as 0): the room's outbound bytes of this sweep */
  uint64_t        wire_cap;
} xyws_room;

typedef struct xyws_room_result {     /* 32 bytes */
  uint64_t wire_len;   /* full length of the room's wire (may exceed wire_cap) */
  uint32_t nmsgs;      /* messages framed onto it */
  uint32_t skipped;    /* stored records of its members that were not delivered */
  uint32_t receivers;  /* members that receive the wire */
  uint32_t status;     /* XYWS_ROOM_* */
  uint64_t reserved;
} xyws_room_result;
#define XYWS_ROOM_TRUNCATED  0x1u /* wire_len > wire_cap */
#define XYWS_ROOM_BAD_MEMBER 0x2u /* a members[] entry >= n: ignored, never dereferenced */
#define XYWS_ROOM_MSG_CAP    0x4u /* a member had nmsgs > msg_cap: unstored records cannot be delivered */

typedef struct xyws_bcast_conn {      /* 64 bytes; entry i goes with dev_reasm[i] */
  const void* head;      /* device, nullable: bytes put before each of this connection's messages
                            (chat_session::make_message_head, websocket_chat.cpp:139-146) */
  uint64_t    head_len;  /* 0 when head is NULL */
  void*       out;       /* device: this connection's send buffer (the one xyws_reply_streams wrote) */
  uint64_t    out_cap;
  const xyws_reply_result* reply; /* device, nullable: this connection's row of the same sweep's reply call */
  uint32_t    room;      /* index into dev_rooms, or XYWS_ROOM_NONE; >= n_rooms counts as NONE */
  uint32_t    reserved0;
  uint64_t    reserved[2];
} xyws_bcast_conn;

typedef struct xyws_bcast_result {    /* 32 bytes */
  uint64_t send_len;   /* base + bcast_len: the caller sends out[0 .. min(send_len, out_cap)) */
  uint64_t bcast_len;  /* bytes of the room's wire appended for this connection */
  uint32_t status;     /* XYWS_BC_* */
  uint32_t reserved0;
  uint64_t reserved;
} xyws_bcast_result;
#define XYWS_BC_TRUNCATED    0x1u /* send_len > out_cap */
#define XYWS_BC_NOT_RECEIVER 0x2u /* closed or overflowed: nothing appended */
#define XYWS_BC_NO_ROOM      0x4u

int xyws_broadcast_streams(xyws_ctx* ctx,
                           const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                           const xyws_bcast_conn* dev_bconns, uint64_t n,
                           const xyws_room* dev_rooms, xyws_room_result* dev_room_results, uint64_t n_rooms,
                           uint8_t flags, uint32_t enc_opts,
                           xyws_bcast_result* dev_results /* n, nullable */, void* stream);

/* ---- many connections, one hold call ---------------------------------------
 * The message a recv boundary cut: xyws_reassemble_streams reports it as an
 * open record in one sweep and as XYWS_MSG_CONTINUED records in the next, and
 * xyws_broadcast_streams delivers neither. This call, between the two, keeps
 * the parts of such a message in a per-connection hold on the device and, in
 * the sweep that completes it, hands the broadcast a view of the reassembly
 * table in which the whole message is one ordinary record: decode, reassemble,
 * hold, reply, broadcast, still with no host read of device state. dev_reasm
 * and dev_reasm_results are the table and rows of this sweep's
 * xyws_reassemble_streams call; dev_view and dev_view_results (n entries each)
 * are written here and passed to xyws_broadcast_streams in their place. The
 * call is independent of xyws_reply_streams.
 *
 * Where the hold lives. The hold of connection i is the hold_cap bytes
 * immediately in front of its reassembly range: hold = out - hold_cap. The
 * caller allocates one area per connection and gives xyws_reassemble_streams
 * out = area + hold_cap (that call never writes in front of out), so the view
 * names hold and message bytes with one base. With H = (hold_cap / 2) & ~15
 * the hold is used as two halves [0, H) and [H, 2H): a held message never
 * exceeds H, and a message delivered from one half stays readable there while
 * the next one begins in the other. hold_cap >= 2 * (largest message accepted)
 * + 30 always suffices (H rounds hold_cap / 2 down to a 16-byte line).
 *
 * Per connection, with s = min(nmsgs, msg_cap) (0 for a null msgs) and the
 * carry hc:
 *
 *  0. Pass-through. out NULL, hc NULL or H == 0: dev_view[i] and
 *     dev_view_results[i] are the inputs copied verbatim, the result is
 *     {0, 0, XYWS_HOLD_PASSTHROUGH}; nothing else is touched.
 *  1. The view. Otherwise dev_view[i] = {out - hold_cap, hold_cap + out_cap,
 *     mc, vmsgs, min(msg_cap, vmsg_cap), 0...} (a null vmsgs counts as
 *     vmsg_cap 0) and dev_view_results[i] is the input row, with
 *     XYWS_RSM_MSG_CAP added when s > vmsg_cap. View record j, j <
 *     min(s, vmsg_cap), is record j with out_off += hold_cap; the one
 *     exception is the delivered record of step 3.
 *  2. Overflow. The row has XYWS_RSM_OVERFLOW: the carry becomes
 *     {status = LOST} and stays so, as XYWS_MSG_OVERFLOW does (DROPPED when a
 *     message was held).
 *  3. Record 0 with XYWS_MSG_CONTINUED (stored). With an ACTIVE carry the
 *     record's bytes out[out_off .. +length) are appended at
 *     hold[start + held ..), held += length, nframes += the record's. If the
 *     record has TRUNCATED, or out_off + length > out_cap, or held + length >
 *     H, the message becomes LOST instead and nothing is copied: the result
 *     has DROPPED, and TOO_LONG in the last of those cases (the caller closes
 *     with 1009). An ACTIVE carry whose start is neither 0 nor H or whose held
 *     exceeds H (a hold_cap that changed between sweeps) is LOST and DROPPED
 *     likewise. A carry neither ACTIVE nor LOST (attached mid-message) becomes
 *     LOST and DROPPED. Then, if the record has COMPLETE: an ACTIVE message is
 *     delivered: view record 0 is {first_frame 0, nframes = carry.nframes,
 *     out_off = start, length = held, status = the record's without
 *     CONTINUED, the carry's opcode}, the result has DELIVERED and
 *     delivered_len = held, the carry clears; a LOST message clears, its view
 *     record stays CONTINUED and the broadcast skips it as before. With
 *     INTERRUPTED the carry clears and nothing is delivered. UTF8_BAD and
 *     UNCHECKED ride along in the status: the broadcast's own rule then skips
 *     a bad message.
 *  4. The message open at the end. The row has XYWS_RSM_OPEN and record
 *     nmsgs - 1 is stored, is not CONTINUED and has neither COMPLETE nor
 *     INTERRUPTED: it starts a hold in the half the message delivered by this
 *     call does not occupy (half 0 if none was): its bytes
 *     out[out_off .. +length) go to hold[target ..), the carry becomes
 *     {start = target, held = length, nframes, ACTIVE, opcode}. With TRUNCATED,
 *     out_off + length > out_cap, or length > H the carry becomes LOST, the
 *     result has DROPPED, and TOO_LONG in the last case.
 *  5. Closing rule (records msg_cap did not store). An ACTIVE carry whose
 *     record 0 is not a stored CONTINUED record becomes LOST (DROPPED). After
 *     the walk: with XYWS_RSM_OPEN set a carry neither ACTIVE nor LOST becomes
 *     LOST (DROPPED); with it clear the carry clears. The carry is exact
 *     whatever vmsg_cap. The result row is {carry.held, delivered_len, the
 *     bits above | the carry's ACTIVE and LOST}.
 *  6. Bounds. Nothing outside [out, out + out_cap) is read as message bytes
 *     (whole 16-byte lines that hold one of them are loaded); nothing outside
 *     the part of the hold a copy names is written: whole lines inside it,
 *     byte stores on its first and last line (neighbouring connections' areas
 *     may abut, every alignment of out, hold_cap and out_off is legal); view
 *     records at index >= min(s, vmsg_cap) are never written.
 *
 * Known approximation: the delivered record has first_frame 0, so the
 * broadcast's rule first_frame < first_close drops it in the one sweep whose
 * frame 0 is the close frame.
 *
 * Like its siblings the call is one launch (one wave per connection), uses no
 * context scratch, no scratch slot and no policy word, never touches the
 * device error word, reads no device state on the host, needs no reserve, can
 * be captured into a hipGraph at once and runs concurrently on different
 * streams. n == 0 returns XYWS_OK and launches nothing. XYWS_ERR_INVALID: a
 * null ctx; a null dev_reasm, dev_reasm_results, dev_hold, dev_view or
 * dev_view_results with n > 0; decided on the arguments alone. The areas must
 * not overlap; a hold carry or a view row must not appear twice in a call;
 * vmsgs must not be the reassembly's msgs. */
typedef struct xyws_hold_carry {     /* 32 bytes; all zero = nothing held */
  uint64_t start;    /* the half in use: 0 or H */
  uint64_t held;     /* bytes of the open message in hold[start ..) */
  uint64_t nframes;  /* its data frames so far */
  uint32_t status;   /* XYWS_HOLD_ACTIVE or XYWS_HOLD_LOST; without ACTIVE every other field is zero */
  uint8_t  opcode;   /* XYWS_FLAG_OP_TEXT / _BINARY of the held message */
  uint8_t  reserved[3];
} xyws_hold_carry;

typedef struct xyws_hold_conn {      /* 32 bytes; entry i goes with dev_reasm[i] */
  uint64_t         hold_cap; /* bytes in front of dev_reasm[i].out that are this connection's hold */
  xyws_hold_carry* hc;       /* device; read, then written. NULL: pass-through */
  xyws_message*    vmsgs;    /* device, nullable (then vmsg_cap counts as 0): the view's record row */
  uint64_t         vmsg_cap;
} xyws_hold_conn;

typedef struct xyws_hold_result {    /* 32 bytes */
  uint64_t held;          /* the carry's after this call */
  uint64_t delivered_len; /* length of the message this call delivered (0: none) */
  uint32_t status;        /* XYWS_HOLD_* */
  uint32_t reserved0;
  uint64_t reserved;
} xyws_hold_result;
#define XYWS_HOLD_DELIVERED   0x1u  /* view record 0 is a whole message out of the hold */
#define XYWS_HOLD_ACTIVE      0x2u  /* carry and result: a message is held */
#define XYWS_HOLD_LOST        0x4u  /* carry and result: the open message cannot be delivered */
#define XYWS_HOLD_DROPPED     0x8u  /* this call lost a message */
#define XYWS_HOLD_TOO_LONG    0x10u /* ... because it exceeds H: the caller closes with 1009 */
#define XYWS_HOLD_PASSTHROUGH 0x20u

int xyws_hold_streams(xyws_ctx* ctx,
                      const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                      const xyws_hold_conn* dev_hold, uint64_t n,
                      xyws_reasm_conn* dev_view, xyws_reasm_result* dev_view_results,
                      xyws_hold_result* dev_results /* n, nullable */, void* stream);

/* ---- many rooms, one backlog call -------------------------------------------
 * The room's memory: chat_room::deliver keeps the last 10 messages in
 * m_recent_messages and chat_room::join sends them to every newcomer through
 * deliver_recent_messages (example/websocket/websocket_chat.cpp:34-47, 89-95).
 * Here a room's framed wire exists only for one sweep. This call, after
 * xyws_broadcast_streams, folds the sweep's newest frames into a per-room
 * backlog on the device and copies the backlog behind the send bytes of every
 * connection marked as joining: decode, reassemble, hold, reply, broadcast,
 * backlog, still with no host read of device state. The welcome and farewell
 * lines of the reference's room (:49-87) are server-authored text:
 * xyws_roster_streams (below), called between the broadcast and this call,
 * frames and delivers them, and this call appends behind them.
 *
 * dev_reasm, dev_reasm_results, dev_bconns, n, dev_rooms and n_rooms are what
 * this sweep's xyws_broadcast_streams call was given (the hold's view when
 * there is one), dev_room_results the rows that call wrote. dev_brooms[r] goes
 * with dev_rooms[r], dev_jconns[i] with dev_bconns[i].
 *
 * The log. With H = (log_cap / 2) & ~15 the log is used as two halves [0, H)
 * and [H, 2H), as the hold is: a fold writes the half the backlog does not
 * occupy, so the copy never overlaps its source. With B the most bytes the
 * backlog is to hold, log_cap >= 2 * B + 30 always gives H >= B.
 *
 *  0. Pass-through. log NULL, bc NULL, keep == 0 or H == 0: neither the log
 *     nor the carry is touched, the room result is
 *     {0, 0, 0, 0, XYWS_BL_PASSTHROUGH} and the room's joiners get nothing.
 *
 * The fold, per room, N = dev_room_results[r].nmsgs, the bytes out of the
 * room's wire:
 *
 *  1. No new message. N == 0: the carry and the log stay as they are (the
 *     carry is not checked), and the row reports the carry's len and count.
 *  2. The carry is valid when start is 0 or H, len <= H, count <=
 *     XYWS_BACKLOG_MAX and the first count entries of flen[] sum to len.
 *     Anything else counts as empty (gaps and total are kept) and sets
 *     XYWS_BL_BAD_CARRY.
 *  3. The new frames are the room's deliverable records (xyws_broadcast_streams
 *     2. and 3.) in wire order. A frame's size is the header size for head_len
 *     + length (2, 4 or 10 bytes) plus head_len + length; flags do not enter
 *     it. The call recounts and resizes them from the tables: when the count
 *     differs from the room row's nmsgs or the total from its wire_len, the
 *     caller passed other tables and the backlog is cleared with
 *     XYWS_BL_MISMATCH | XYWS_BL_GAP.
 *  4. Truncated wire. The room row has XYWS_ROOM_TRUNCATED (or wire_len >
 *     wire_cap): the newest frames cannot be read, the backlog is cleared with
 *     XYWS_BL_GAP.
 *  5. Selection. The candidates are the old frames, oldest first, then the N
 *     new ones. From the newest backwards a frame is taken while fewer than
 *     keep are taken (keep > XYWS_BACKLOG_MAX counts as it) and the bytes
 *     taken plus its size stay <= H; the walk stops at the first frame that
 *     fails either test, the count test first. When the byte budget ended it,
 *     XYWS_BL_EVICTED is set; when the newest frame alone exceeds H the
 *     backlog ends empty and XYWS_BL_TOO_LONG is set too.
 *  6. Copy. target = H when the valid carry had count > 0 and start == 0 and
 *     the backlog does not end empty, else 0. The surviving old bytes are a
 *     suffix of the old half's held bytes, the surviving new bytes the suffix
 *     wire[wire_len - b .. wire_len); both go to log[target ..), old first.
 *  7. The carry becomes {target, bytes, count, gaps, total + folded, flen
 *     oldest first, zeros}; gaps counts XYWS_BL_GAP events. Every clear, and a
 *     backlog that ends empty, leaves start, len, count and flen zero. The
 *     room row is {len, count, folded = new frames taken, dropped = old frames
 *     let go, status}; a clear folds none and drops every old frame.
 *  8. Bounds. Nothing outside the part of the half a copy names is written:
 *     whole 16-byte lines inside it, byte stores on its first and last line.
 *     Every alignment of log, wire and both suffixes is legal, neighbouring
 *     rooms' logs may abut. Nothing outside [wire, wire + wire_cap) and the
 *     old half's held bytes is read, apart from the whole lines that hold
 *     them. Logs, wires and send buffers must not overlap.
 *
 * Delivery, per connection with XYWS_BL_JOIN in flags, after the fold (a
 * joiner sees this sweep's talk):
 *
 *  9. base = bcast ? bcast->send_len : reply ? reply->reply_len : 0. A room >=
 *     n_rooms or a pass-through room: {base, 0, XYWS_BLC_NO_ROOM}. Otherwise,
 *     when reply has CLOSED or OVERFLOW or bcast has XYWS_BC_NOT_RECEIVER:
 *     {base, 0, XYWS_BLC_NOT_RECEIVER}. Otherwise log[start .. start + len)
 *     goes to out + base (a carry whose start is neither 0 nor H or whose len
 *     exceeds H counts as len 0); positions >= out_cap are not written;
 *     backlog_len = len, send_len = base + len, XYWS_BLC_JOINED is set, and
 *     XYWS_BLC_TRUNCATED when send_len > out_cap. A connection without the
 *     flag gets {base, 0, 0} and nothing written. No byte outside
 *     [out + min(base, out_cap), out + min(send_len, out_cap)) is written:
 *     send-slab neighbours share lines.
 * 10. The caller's duty. A joiner is added to its room's members[] from the
 *     next sweep on. If it is a member already it receives the wire and the
 *     same frames again in the backlog. That is the reference's order with the
 *     join placed after the sweep's messages: the last keep messages, then
 *     everything later.
 * 11. Properties. At most two launches on `stream`: the fold (one workgroup
 *     per room; omitted when n_rooms == 0), then the delivery (omitted when
 *     dev_jconns is NULL or n == 0); the carries are the hand-over between
 *     them. Like its siblings the call uses no context scratch, no scratch
 *     slot and no policy word, never touches the device error word, reads no
 *     device state on the host, needs no reserve, can be captured into a
 *     hipGraph at once and runs concurrently on different streams. n == 0 &&
 *     n_rooms == 0 returns XYWS_OK and launches nothing. XYWS_ERR_INVALID: a
 *     null ctx; null dev_reasm, dev_reasm_results or dev_bconns with n > 0 and
 *     n_rooms > 0; null dev_rooms, dev_room_results or dev_brooms with n_rooms
 *     > 0; n >= UINT32_MAX. Every refusal is decided on the arguments alone,
 *     before the context is used. */
#define XYWS_BACKLOG_MAX 16u            /* the reference keeps 10 */

typedef struct xyws_backlog_carry {     /* 192 bytes; all zero = empty */
  uint64_t start;      /* the half of the log in use: 0 or H */
  uint64_t len;        /* bytes held: whole server frames, oldest first */
  uint32_t count;      /* frames held, <= XYWS_BACKLOG_MAX */
  uint32_t gaps;       /* times the history was lost (XYWS_BL_GAP) */
  uint64_t total;      /* frames folded in over all calls */
  uint64_t flen[XYWS_BACKLOG_MAX]; /* their lengths, oldest first; zero from count on */
  uint64_t reserved[4];
} xyws_backlog_carry;

typedef struct xyws_backlog_room {      /* 32 bytes; entry r goes with dev_rooms[r] */
  void*               log;      /* device, any alignment */
  uint64_t            log_cap;
  xyws_backlog_carry* bc;       /* device; read, then written */
  uint32_t            keep;     /* frames to keep; > XYWS_BACKLOG_MAX counts as it */
  uint32_t            reserved0;
} xyws_backlog_room;

typedef struct xyws_backlog_room_result { /* 32 bytes */
  uint64_t len;        /* the carry's after this call */
  uint32_t count;      /* the carry's after this call */
  uint32_t folded;     /* new frames taken */
  uint32_t dropped;    /* old frames let go */
  uint32_t status;     /* XYWS_BL_* */
  uint64_t reserved;
} xyws_backlog_room_result;
#define XYWS_BL_PASSTHROUGH 0x1u
#define XYWS_BL_BAD_CARRY   0x2u  /* the carry was not valid: counted as empty */
#define XYWS_BL_MISMATCH    0x4u  /* the tables are not the ones the room row was made from */
#define XYWS_BL_GAP         0x8u  /* the history was lost: the backlog is cleared */
#define XYWS_BL_EVICTED     0x10u /* the byte budget H, not keep, ended the selection */
#define XYWS_BL_TOO_LONG    0x20u /* the newest frame alone exceeds H */

typedef struct xyws_backlog_conn {      /* 64 bytes; entry i goes with dev_bconns[i] */
  void*    out;        /* device: the connection's send buffer */
  uint64_t out_cap;
  const xyws_bcast_result* bcast; /* device, nullable: this sweep's broadcast row */
  const xyws_reply_result* reply; /* device, nullable: this sweep's reply row */
  uint32_t room;       /* the room joined; >= n_rooms counts as none */
  uint32_t flags;      /* XYWS_BL_JOIN */
  uint64_t reserved[3];
} xyws_backlog_conn;
#define XYWS_BL_JOIN 0x1u

typedef struct xyws_backlog_result {    /* 32 bytes */
  uint64_t send_len;    /* base + backlog_len: the caller sends out[0 .. min(send_len, out_cap)) */
  uint64_t backlog_len; /* bytes of the room's backlog appended for this connection */
  uint32_t status;      /* XYWS_BLC_* */
  uint32_t reserved0;
  uint64_t reserved;
} xyws_backlog_result;
#define XYWS_BLC_JOINED       0x1u
#define XYWS_BLC_TRUNCATED    0x2u /* send_len > out_cap */
#define XYWS_BLC_NO_ROOM      0x4u /* no such room, or a pass-through room */
#define XYWS_BLC_NOT_RECEIVER 0x8u /* closed or overflowed: nothing appended */

int xyws_backlog_streams(xyws_ctx* ctx,
                         const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                         const xyws_bcast_conn* dev_bconns, uint64_t n,
                         const xyws_room* dev_rooms, const xyws_room_result* dev_room_results,
                         const xyws_backlog_room* dev_brooms,
                         xyws_backlog_room_result* dev_broom_results /* n_rooms, nullable */, uint64_t n_rooms,
                         const xyws_backlog_conn* dev_jconns /* n, nullable: fold only */,
                         xyws_backlog_result* dev_results /* n, nullable */, void* stream);

/* ---- many connections, one opening handshake call ---------------------------
 * xyws_accept_streams: the HTTP upgrade of every connection still in HTTP
 * state, answered by one launch (the reference's websocket_request_handler
 * over http_parser / picohttpparser, include/xynet/http/websocket_request_handler.h,
 * as websocket_handshake drives it, example/include/common/websocket.h:40-68).
 * It is the first call in a connection's life and keeps no state: entry i
 * names every byte connection i has sent so far, from its first, and its
 * send buffer. With E = min(len, max_request) the verdict is a pure function
 * of buf[0, E), policy and whether len >= max_request.
 *
 *  1. Grammar. picohttpparser's phr_parse_request as a fresh parser runs it,
 *     defined by its sequential walk from byte 0; the first event decides:
 *     a grammar error before byte E is REJECTED with reason PARSE, the end of
 *     the bytes is incomplete (neither ACCEPTED nor REJECTED: call again with
 *     more bytes; nothing is written), the blank line ends the request and
 *     nothing behind it is looked at. Incomplete with len >= max_request is
 *     REJECTED with reason TOO_LONG. The walk: one optional leading empty
 *     line; LF-only line ends everywhere; method and target end at SP, reject
 *     bytes < 0x20 and 0x7f, take bytes >= 0x80, and are non-empty; runs of SP
 *     between the three parts (the end of the bytes is not a space); the
 *     version wants 9 bytes left (else incomplete, whatever they are) and is
 *     `HTTP/1.` and a digit; header names are token characters up to `:`
 *     (empty, or SP before the colon: error); SP/HT after the colon skipped;
 *     the value runs to CR LF or LF, another byte < 0x20 except HT, or 0x7f,
 *     is an error, a CR as the last byte is incomplete, trailing SP/HT are
 *     trimmed; a line that begins with SP/HT after the first header is a
 *     nameless continuation ("folded"); a 101st header is an error.
 *  2. Policy 0 applies RFC 6455 4.2.1 to the parsed request. The checks, in
 *     the order of their XYWS_ACR_* codes (the lowest failing one is
 *     reported): method GET; minor version >= 1; no folded line; a Host
 *     header (names are matched ASCII case-insensitively); an Upgrade header
 *     with a comma-separated element equal to `websocket` (case-insensitive,
 *     SP/HT trimmed); a Connection header with an element `upgrade` by the
 *     same rule; Sec-WebSocket-Key exactly once, 24 bytes: 21 base64
 *     characters, one of `AQgw`, `==`; Sec-WebSocket-Version exactly once and
 *     equal to `13`. Responses: 101 (129 bytes, below); 426 when the version
 *     check is the lowest failing one (`HTTP/1.1 426 Upgrade Required`,
 *     `Sec-WebSocket-Version: 13`, `Connection: close`, `Content-Length: 0`,
 *     98 bytes); else 400 (`HTTP/1.1 400 Bad Request`, `Connection: close`,
 *     `Content-Length: 0`, 66 bytes).
 *  3. XYWS_ACC_REFERENCE is websocket_request_handler::generate_response,
 *     bugs included: method exactly GET, minor version exactly 1; of the
 *     headers before the first folded line (http_parser::headers() ends
 *     there) those named exactly `Connection`, `Upgrade`,
 *     `Sec-WebSocket-Version`, `Sec-WebSocket-Key` are checked against
 *     `Upgrade`, `websocket`, `13`, and a length of 24; absent headers are not
 *     missed. Any 24 key bytes pass, the last occurrence is hashed, and with
 *     no key the placeholder `XXXXXXXXXXXXXXXXXXXXXX==` is. Responses: the
 *     same 101; the reference's 26-byte `HTTP/1.1 400 Bad Request\r\n` (no
 *     blank line). One departure: the reference answers an incomplete request
 *     with that 400; here incomplete is reported as incomplete.
 *  4. The 101 response is `HTTP/1.1 101 Switching Protocols`, `Upgrade:
 *     websocket`, `Connection: Upgrade`, `Sec-WebSocket-Accept: ` + base64(
 *     SHA-1(key + 258EAFA5-E914-47DA-95CA-C5AB0DC85B11)), blank line.
 *     Subprotocols and extensions are ignored and never negotiated.
 *  5. Nothing outside buf[0, E) is read but the whole 16-byte lines that hold
 *     one of those bytes; no byte outside [out, out + min(resp_len, out_cap))
 *     is written (neighbouring ranges share 16-byte lines); buffers may have
 *     any alignment. resp_len is the full length; TRUNCATED when it exceeds
 *     out_cap.
 *  6. One launch, no context scratch, no host read of device state; no
 *     reserve is needed, the call can be captured into a hipGraph at once and
 *     runs concurrently on different streams. n == 0 returns XYWS_OK and
 *     launches nothing. XYWS_ERR_INVALID: a null ctx; null dev_conns with
 *     n > 0; max_request 0 or above XYWS_ACCEPT_MAX_REQUEST; unknown policy
 *     bits.
 *
 * xyws_accept_request is the same function of one request in host memory:
 * the same source compiled for the host, no context and no HIP call. */
#define XYWS_ACCEPT_MAX_REQUEST 8192u /* a whole request fits one wave's LDS */
#define XYWS_ACC_ACCEPTED   0x1u /* xyws_accept_result.status */
#define XYWS_ACC_REJECTED   0x2u
#define XYWS_ACC_TRUNCATED  0x4u /* resp_len > out_cap */
#define XYWS_ACC_REFERENCE  0x100u /* policy bit */
#define XYWS_ACR_NONE        0
#define XYWS_ACR_PARSE       1
#define XYWS_ACR_TOO_LONG    2
#define XYWS_ACR_METHOD      3
#define XYWS_ACR_VERSION     4
#define XYWS_ACR_FOLDED      5
#define XYWS_ACR_HOST        6
#define XYWS_ACR_UPGRADE     7
#define XYWS_ACR_CONNECTION  8
#define XYWS_ACR_KEY         9
#define XYWS_ACR_WS_VERSION 10

typedef struct xyws_accept_conn {   /* 32 bytes */
  const void* buf;     /* device: every byte this connection has sent so far, from its first */
  uint64_t    len;     /* 0 allowed: incomplete, nothing written */
  void*       out;     /* device: its send buffer; nullable with out_cap 0 */
  uint64_t    out_cap;
} xyws_accept_conn;

typedef struct xyws_accept_result { /* 32 bytes */
  uint32_t status;      /* XYWS_ACC_ACCEPTED | XYWS_ACC_REJECTED | XYWS_ACC_TRUNCATED; neither of the first two: incomplete */
  uint16_t http_status; /* 101, 400, 426, or 0 while incomplete */
  uint16_t reason;      /* XYWS_ACR_*: 0 when accepted or incomplete, else the lowest-numbered failing check */
  uint32_t consumed;    /* accepted: bytes of the request, its blank line included (buf + consumed is the
                           connection's first frame byte: a valid xyws_conn.buf, any alignment); the same
                           for a whole request that a check refused (reason >= XYWS_ACR_METHOD); else 0 */
  uint32_t resp_len;    /* full length of the response, whatever out_cap */
  uint32_t path_off;    /* the request target, for routing; 0, 0 unless accepted */
  uint32_t path_len;
  uint32_t key_off;     /* accepted: offset of the 24 key bytes that were hashed; UINT32_MAX if none */
  uint32_t reserved;
} xyws_accept_result;

int xyws_accept_streams(xyws_ctx* ctx, const xyws_accept_conn* dev_conns, uint64_t n,
                        uint32_t max_request, uint32_t policy,
                        xyws_accept_result* dev_results /* n, nullable */, void* stream);
int xyws_accept_request(const void* host_req, uint64_t len, uint32_t max_request, uint32_t policy,
                        void* host_out, uint64_t out_cap, xyws_accept_result* res /* nullable */);

/* ---- many rooms, one roster call ---------------------------------------------
 * Who is in the room: chat_room::m_participants with join and leave, and the
 * welcome and farewell lines the room says on each (example/websocket/
 * websocket_chat.cpp:34-39, 49-87). This call, between xyws_broadcast_streams
 * and xyws_backlog_streams, keeps every room's member list on the device. It
 * takes the sweep's joins and leaves from the sweep's own result rows, rewrites
 * the lists the next sweep's broadcast reads, frames one notice per event into
 * the room's notice wire, delivers that wire as the broadcast delivers the
 * room's wire, and marks the joiners for the backlog call: accept, decode,
 * reassemble, hold, reply, broadcast, roster, backlog, with no host read of
 * device state. A connection whose handshake completes in a sweep is sent
 * `101 | welcome | recent messages` in that sweep.
 *
 * dev_bconns, n, dev_rooms and n_rooms are the broadcast's tables;
 * dev_rconns[i] goes with dev_bconns[i], dev_rrooms[r] with dev_rooms[r]. The
 * member arrays dev_rooms[r].members names must be writable and hold
 * member_cap entries. text is a host pointer, copied into the launches; NULL
 * means the reference's three strings. flags are a notice's frame flags, as
 * xyws_broadcast_streams takes them.
 *
 *  1. Events. With rc = dev_rconns[i]: connection i leaves when rc.flags has
 *     XYWS_RS_LEAVE, or has XYWS_RS_LEAVE_ON_CLOSE while rc.reply is given and
 *     has XYWS_RPL_CLOSED. A leave has an effect only where a room's list holds
 *     i. Connection i wants to join rc.room when it does not leave, rc.room <
 *     n_rooms, and rc.flags has XYWS_RS_JOIN, or has XYWS_RS_JOIN_ON_ACCEPT
 *     while rc.accept is given and has XYWS_ACC_ACCEPTED. A connection with
 *     dev_bconns[i].room < n_rooms counts as a member of that room: its join is
 *     refused with XYWS_RSC_ALREADY and nothing changes. Leave wins over join.
 *     A null name has length 0 whatever name_len says; a name_len above
 *     XYWS_ROSTER_NAME_MAX counts as 0 and sets XYWS_RSC_BAD_NAME. The event
 *     still happens: no member gets stuck in a list because of its name.
 *  2. The list, per room r. First the leavers and the entries >= n
 *     (XYWS_RS_BAD_MEMBER: dropped, never dereferenced) are removed, the
 *     others keeping their order. Then the room's joiners are appended in
 *     ascending table index while n_members < member_cap (0 for a null
 *     members); the others get XYWS_RSC_FULL, no welcome and no table change
 *     (the room row gets XYWS_RS_FULL; the caller raises XYWS_RS_JOIN again or
 *     closes them). dev_rooms[r].n_members is rewritten. dev_bconns[i].room
 *     becomes r for an admitted joiner and XYWS_ROOM_NONE for a leaver that was
 *     listed; of both rows only these fields are written. The new list is what
 *     the next sweep's broadcast reads: the join protocol of
 *     xyws_backlog_streams 10.
 *  3. The notice wire of room r: the farewells of its leavers in the order
 *     members[] had them, then the welcomes of its admitted joiners in joining
 *     order. A notice is header(flags, L) | head | name_i | joined-or-left with
 *     L = head_len + name_len_i + the tail's length, the header as
 *     xyws_broadcast_streams builds it (2 bytes for L < 126, else 4). Positions
 *     >= notes_cap (0 for a null notes) are not written; notes_len,
 *     welcome_off = the farewells' length, joined, left and n_members are exact
 *     whatever notes_cap; XYWS_RS_TRUNCATED is set when notes_len > notes_cap.
 *     No byte outside [notes, notes + min(notes_len, notes_cap)) is written.
 *  4. Delivery. base = bcast ? bcast->send_len : reply ? reply->reply_len :
 *     accept ? (ACCEPTED or REJECTED ? resp_len : 0) : 0. Not a receiver:
 *     reply has CLOSED or OVERFLOW; bcast has XYWS_BC_NOT_RECEIVER; every
 *     leaver; a connection with XYWS_RS_JOIN_ON_ACCEPT whose accept row is
 *     given and not ACCEPTED. Its row is {base, 0, XYWS_RSC_NOT_RECEIVER | the
 *     event bits}. Otherwise, with w = min(notes_len, notes_cap) of its room: a
 *     member that stays (XYWS_RSC_MEMBER) receives notes[0 .. w), note_off 0;
 *     an admitted joiner (XYWS_RSC_JOINED) the suffix that begins at its own
 *     welcome: note_off is that offset, note_len = max(w - note_off, 0). That
 *     is what the reference's sequential leave.., join.. sends each
 *     participant when the sweep's leaves are placed before its joins: whoever
 *     is present hears every farewell and every welcome, a newcomer its own
 *     welcome and the later ones. Everyone else gets {base, 0,
 *     XYWS_RSC_NO_ROOM | the event bits}. The bytes go to out + base; positions
 *     >= out_cap (0 for a null out) are not written; send_len = base +
 *     note_len, XYWS_RSC_TRUNCATED whenever send_len > out_cap. room
 *     is the room the connection is in after the call, for a listed leaver the
 *     room it left, else XYWS_ROOM_NONE. No byte outside
 *     [out + min(base, out_cap), out + min(send_len, out_cap)) is written:
 *     send-slab neighbours share 16-byte lines, and out, notes and name may
 *     have any alignment.
 *  5. Hand-over to the backlog. With dev_jconns given, room and flags of entry
 *     i become {r, XYWS_BL_JOIN} for an admitted joiner and {XYWS_ROOM_NONE, 0}
 *     for every other connection; nothing else of the row is written. A roster
 *     row has send_len, note_len and status where xyws_bcast_result has
 *     send_len, bcast_len and status, and XYWS_RSC_TRUNCATED, _NOT_RECEIVER and
 *     _NO_ROOM have the XYWS_BC_ values: the caller sets dev_jconns[i].bcast =
 *     &dev_results[i] once and the backlog appends behind the notices,
 *     unchanged. Notices are not folded into the backlog (welcome and farewell
 *     bypass m_recent_messages too).
 *     The lists this sweep's backlog folds. xyws_backlog_streams recounts the
 *     room's frames from the list the broadcast read and clears the backlog
 *     (XYWS_BL_MISMATCH | XYWS_BL_GAP) when the count differs from the room row:
 *     after this call dev_rooms no longer is that list wherever a member that
 *     spoke left (it said something and closed in the same sweep) or a joiner
 *     had messages of its own in the sweep's tables. So this sweep's backlog
 *     call is given the `seen` rows in place of dev_rooms: with
 *     dev_rrooms[r].seen set, seen->members[0 .. c) receives members[0 .. c)
 *     as this call found them, c = min(n_members, member_cap), bad entries
 *     included, and seen->n_members = c, before anything is rewritten; wire
 *     and wire_cap of the seen row are the caller's (the same as
 *     dev_rooms[r]'s) and are not touched. The seen rows of all rooms form one
 *     table, entry r for room r; their member arrays are not the rooms' own.
 *     A caller that passes dev_rooms itself to the backlog after this call
 *     loses the backlog of every room in which one of the two cases occurs.
 *  6. The caller's duties. A member keeps its table index for as long as it is
 *     listed (an idle connection is an entry with len = 0); a slot is free
 *     again in the sweep after its leave. dev_rooms, dev_bconns and the member
 *     arrays stay resident on the device and are not uploaded again over this
 *     call's writes. A connection is listed at most once and
 *     dev_bconns[i].room names the room that lists it. notes, the wires, the
 *     logs and the send buffers must not overlap. When the caller breaks these
 *     the results are unspecified; nothing outside the named ranges is touched.
 *  7. Properties. At most three launches on `stream`: the events (one thread
 *     per connection: fills dev_want and initialises every result row; omitted
 *     when n == 0), the room pass (one workgroup per room: 2. and 3.; omitted
 *     when n_rooms == 0) and the delivery (omitted when n == 0); dev_want and
 *     dev_results are the hand-over between them. No context scratch, no
 *     atomics, nothing spins; the device error word is untouched; no device
 *     state is read on the host; no reserve is needed; the call can be captured
 *     into a hipGraph at once and runs concurrently on different streams.
 *     n == 0 && n_rooms == 0 returns XYWS_OK and launches nothing.
 *     XYWS_ERR_INVALID, decided on the arguments alone before the context is
 *     used: a null ctx; null dev_bconns, dev_rconns, dev_want or dev_results
 *     with n > 0; null dev_rooms, dev_rrooms or dev_room_results with n_rooms >
 *     0; n >= UINT32_MAX or n_rooms >= UINT32_MAX (indices are 32 bits); flags
 *     with XYWS_FLAG_HAS_MASK; a text length above 32. */
#define XYWS_ROSTER_NAME_MAX 256u
#define XYWS_ROSTER_TEXT_MAX 32u

typedef struct xyws_roster_conn {        /* 64 bytes; entry i goes with dev_bconns[i] */
  const void* name;      /* device, nullable: the peer's address text (socket_address::to_str()) */
  uint64_t    name_len;  /* <= XYWS_ROSTER_NAME_MAX */
  void*       out;       /* device: the connection's send buffer */
  uint64_t    out_cap;
  const xyws_bcast_result*  bcast;  /* device, nullable: this sweep's rows */
  const xyws_reply_result*  reply;
  const xyws_accept_result* accept;
  uint32_t    room;      /* the room to join */
  uint32_t    flags;     /* XYWS_RS_JOIN | _LEAVE | _JOIN_ON_ACCEPT | _LEAVE_ON_CLOSE */
} xyws_roster_conn;
#define XYWS_RS_JOIN           0x1u
#define XYWS_RS_LEAVE          0x2u
#define XYWS_RS_JOIN_ON_ACCEPT 0x4u
#define XYWS_RS_LEAVE_ON_CLOSE 0x8u

typedef struct xyws_roster_room {        /* 32 bytes; entry r goes with dev_rooms[r] */
  uint64_t member_cap;   /* entries of the writable array dev_rooms[r].members names */
  void*    notes;        /* device, nullable (then notes_cap counts as 0): the room's notice wire of this sweep */
  uint64_t notes_cap;
  xyws_room* seen;       /* device, nullable: a second room row, with a member array of member_cap entries of
                            its own, that receives the list as this call found it (5.) */
} xyws_roster_room;

typedef struct xyws_roster_room_result { /* 32 bytes */
  uint64_t notes_len;    /* full length of the notice wire (may exceed notes_cap) */
  uint64_t welcome_off;  /* where the welcomes begin in it */
  uint32_t joined;       /* joiners admitted */
  uint32_t left;         /* leavers removed */
  uint32_t n_members;    /* the list's length after the call */
  uint32_t status;       /* XYWS_RS_TRUNCATED | _FULL | _BAD_MEMBER */
} xyws_roster_room_result;
#define XYWS_RS_TRUNCATED  0x10u /* notes_len > notes_cap */
#define XYWS_RS_FULL       0x20u /* a joiner was refused for member_cap */
#define XYWS_RS_BAD_MEMBER 0x40u /* a members[] entry >= n: dropped from the list, never dereferenced */

typedef struct xyws_roster_result {      /* 32 bytes; the first three fields lie as xyws_bcast_result's */
  uint64_t send_len;     /* base + note_len: the caller sends out[0 .. min(send_len, out_cap)) */
  uint64_t note_len;     /* bytes of the room's notice wire appended for this connection */
  uint32_t status;       /* XYWS_RSC_* */
  uint32_t room;         /* the room it is in after the call (a listed leaver: the room left), else XYWS_ROOM_NONE */
  uint64_t note_off;     /* where its bytes begin in the notice wire */
} xyws_roster_result;
#define XYWS_RSC_TRUNCATED    0x1u   /* send_len > out_cap */
#define XYWS_RSC_NOT_RECEIVER 0x2u   /* closed, overflowed, leaving or not accepted: nothing appended */
#define XYWS_RSC_NO_ROOM      0x4u
#define XYWS_RSC_MEMBER       0x8u   /* was a member and stays one */
#define XYWS_RSC_JOINED       0x10u
#define XYWS_RSC_LEFT         0x20u
#define XYWS_RSC_FULL         0x40u  /* the join was refused for member_cap */
#define XYWS_RSC_ALREADY      0x80u  /* the join was refused: a member already */
#define XYWS_RSC_BAD_NAME     0x100u /* name_len > XYWS_ROSTER_NAME_MAX: counted as 0 */

typedef struct xyws_roster_text {        /* host; passed to the launches by value */
  uint8_t head[XYWS_ROSTER_TEXT_MAX];    /* before the name */
  uint8_t joined[XYWS_ROSTER_TEXT_MAX];  /* behind it in a welcome */
  uint8_t left[XYWS_ROSTER_TEXT_MAX];    /* behind it in a farewell */
  uint8_t head_len, joined_len, left_len; /* each <= XYWS_ROSTER_TEXT_MAX */
  uint8_t reserved[5];
} xyws_roster_text;

int xyws_roster_streams(xyws_ctx* ctx,
                        xyws_bcast_conn* dev_bconns, const xyws_roster_conn* dev_rconns, uint64_t n,
                        xyws_room* dev_rooms, const xyws_roster_room* dev_rrooms,
                        xyws_roster_room_result* dev_room_results, uint64_t n_rooms,
                        const xyws_roster_text* text /* host, nullable */, uint8_t flags,
                        xyws_backlog_conn* dev_jconns /* n, nullable */,
                        uint32_t* dev_want /* n words of caller scratch */,
                        xyws_roster_result* dev_results /* n */, void* stream);

/* ---- many handshakes, one routing call ----------------------------------------
 * Which room a joiner goes to, decided on the device from the request target
 * (the reference's websocket_request_handler::get_path, which its examples look
 * at on the host). xyws_route_streams runs between xyws_accept_streams and
 * xyws_roster_streams: for every accepted connection it takes the request
 * target out of the request bytes, looks it up in a route table that lives on
 * the device, and writes the room into that connection's roster row, which
 * XYWS_RS_JOIN_ON_ACCEPT then joins: `101 | welcome | recent messages` in the
 * sweep that accepts, whatever the room, with no host read of device state.
 *
 * The table. xyws_route_build makes it on the host as one opaque blob (it begins
 * with a magic and a version word; the hash and the slot layout are private to
 * the library); the caller copies the blob to 4-byte-aligned device memory and
 * passes it to every call. xyws_route_lookup is the same lookup over host
 * memory: the same source compiled for the host, no context and no HIP call.
 *   Normal form: a key loses one trailing `/` when it is longer than one byte.
 *   Bytes are compared as they are: no percent decoding, no case folding, no
 *   dot-segment handling. xyws_route_build refuses with XYWS_ERR_INVALID: a key
 *   of length 0 or above XYWS_ROUTE_KEY_MAX (as given); a key that contains `?`
 *   or `#`; two keys equal in normal form; unknown flags; a non-zero `slots`
 *   that is not a power of two or is <= n_routes (0: the library chooses; the
 *   smallest legal value gives the longest probe chains); null routes with
 *   n_routes > 0, a null key, or a null host_table with cap >= the size needed.
 *   *need receives the blob's size whenever the routes are valid (0 when they
 *   are refused); XYWS_ERR_CAPACITY when cap < *need, and nothing is written.
 *   The key P of a request target T is T up to its first `?` or `#`, in normal
 *   form. Route K matches P when P equals K; a route with XYWS_ROUTE_PREFIX also
 *   when P begins with K and the next byte of P is `/` (for K = `/` it is
 *   enough that P begins with `/`). The longest matching K wins; it is unique.
 *   Only the first XYWS_ROUTE_KEY_MAX bytes of P take part: a longer P has no
 *   exact match, and its prefix candidates are those that end within that
 *   window. `?` and `#` are looked for in the first XYWS_ROUTE_KEY_MAX + 1 bytes
 *   of T only; a target without one there has P = T as it is (its last byte is
 *   not looked at, so key_len is then the target's length).
 *   A damaged blob may misroute, but nothing outside [table, table + table_len)
 *   is ever read: every offset taken from the blob is bounds-checked, on the
 *   host and on the device, and a probe ends after `slots` steps. A blob whose
 *   magic, version or size is wrong (or that is not 4-byte aligned) matches
 *   nothing: every row gets XYWS_RT_BAD_TABLE and is handled as a miss.
 *   table_len == 0 is a table without routes: everything misses.
 *
 * Entry k of dev_rtconns goes with dev_aconns[k] and dev_aresults[k] (the
 * tables of this sweep's xyws_accept_streams call) and names the roster row of
 * that connection.
 *
 *  1. A row whose accept row lacks XYWS_ACC_ACCEPTED is {XYWS_RT_NOT_ACCEPTED,
 *     XYWS_ROOM_NONE, UINT32_MAX, 0, 0}. Nothing else is written for it, not
 *     even its roster row.
 *  2. An accepted row has the key P of buf[path_off, path_off + path_len);
 *     key_off and key_len name P in buf. On a match the status is
 *     XYWS_RT_MATCHED, with XYWS_RT_BY_PREFIX when K is shorter than P; room and
 *     route are the route's room and its index as given to xyws_route_build. On
 *     a miss with policy 0 the status is XYWS_RT_MISS, route UINT32_MAX and
 *     room = default_room, which may be XYWS_ROOM_NONE: accepted, but in no
 *     room. With rconn < n_rconns, dev_rconns[rconn].room = room by one 32-bit
 *     store; no other byte of that row is written. rconn == XYWS_ROUTE_NO_ROW:
 *     only the result row is wanted. Any other rconn >= n_rconns sets
 *     XYWS_RT_BAD_ROW and is never dereferenced. Two entries must not name the
 *     same roster row.
 *  3. A miss under XYWS_RT_MISS_404. The connection's accept row is rewritten to
 *     what xyws_accept_streams writes for a whole request that a check refused:
 *     status XYWS_ACC_REJECTED (| XYWS_ACC_TRUNCATED when out_cap < 64),
 *     http_status 404, reason XYWS_ACR_NOT_FOUND, consumed kept, resp_len 64,
 *     path_off and path_len 0, key_off UINT32_MAX. The 64 bytes `HTTP/1.1 404
 *     Not Found`, `Connection: close`, `Content-Length: 0`, blank line go to
 *     out[0 .. min(64, out_cap)) over the 101; no other byte of out is written
 *     (neighbouring ranges share 16-byte lines). The route row is XYWS_RT_MISS |
 *     XYWS_RT_NOT_FOUND with room XYWS_ROOM_NONE, which is also stored to the
 *     roster row: xyws_roster_streams then treats the connection as a rejected
 *     handshake by its rules 1 and 4, which is why this call runs before it.
 *  4. Reads. Nothing outside buf[path_off, path_off + min(path_len,
 *     XYWS_ROUTE_KEY_MAX + 1)) is read from the request but the whole 16-byte
 *     lines that hold those bytes. The accept row is trusted only as far as
 *     path_off + path_len <= min(len, XYWS_ACCEPT_MAX_REQUEST): a row for which
 *     that does not hold gets XYWS_RT_BAD_ROW and a miss's status, room and
 *     route; nothing is read from its request, and since its tables cannot be
 *     believed nothing but the route row is written for it.
 *  5. One launch, no context scratch, no atomics, no host read of device
 *     state; the device error word is untouched; no reserve is needed, the call
 *     can be captured into a hipGraph at once and runs concurrently on
 *     different streams. n == 0 returns XYWS_OK and launches nothing.
 *     XYWS_ERR_INVALID, decided on the arguments alone: a null ctx; null
 *     dev_aconns, dev_aresults or dev_rtconns with n > 0; a null table with
 *     table_len > 0; null dev_rconns with n_rconns > 0; unknown policy bits. */
#define XYWS_ROUTE_KEY_MAX 256u
#define XYWS_ROUTE_PREFIX  0x1u        /* xyws_route.flags */
#define XYWS_ROUTE_NO_ROW  UINT32_MAX  /* xyws_route_conn.rconn */
#define XYWS_RT_MISS_404   0x1u        /* policy bit */
#define XYWS_RT_MATCHED      0x1u      /* xyws_route_result.status */
#define XYWS_RT_BY_PREFIX    0x2u
#define XYWS_RT_MISS         0x4u
#define XYWS_RT_NOT_FOUND    0x8u      /* the miss was answered with the 404 */
#define XYWS_RT_NOT_ACCEPTED 0x10u
#define XYWS_RT_BAD_ROW      0x20u     /* rconn out of range, or an accept row that names bytes outside the request */
#define XYWS_RT_BAD_TABLE    0x40u
#define XYWS_ACR_NOT_FOUND 11          /* xyws_accept_result.reason after xyws_route_streams' 404 */

typedef struct xyws_route {            /* host; 24 bytes */
  const void* key;
  uint32_t    key_len;   /* 1 .. XYWS_ROUTE_KEY_MAX */
  uint32_t    room;
  uint32_t    flags;     /* XYWS_ROUTE_PREFIX */
  uint32_t    reserved;
} xyws_route;

typedef struct xyws_route_conn {       /* 8 bytes; entry k goes with dev_aconns[k], dev_aresults[k] */
  uint32_t rconn;        /* index into dev_rconns, or XYWS_ROUTE_NO_ROW */
  uint32_t reserved;
} xyws_route_conn;

typedef struct xyws_route_result {     /* 32 bytes */
  uint32_t status;       /* XYWS_RT_* */
  uint32_t room;
  uint32_t route;        /* index given to xyws_route_build, or UINT32_MAX */
  uint32_t key_off;      /* P in buf (in the target for xyws_route_lookup) */
  uint32_t key_len;
  uint32_t reserved[3];
} xyws_route_result;

int xyws_route_build(const xyws_route* routes, uint32_t n_routes, uint32_t slots /* 0: the library chooses */,
                     void* host_table, uint64_t cap, uint64_t* need /* always written when non-null */);
int xyws_route_lookup(const void* host_table, uint64_t table_len, const void* target, uint64_t len,
                      xyws_route_result* res);
int xyws_route_streams(xyws_ctx* ctx, const xyws_accept_conn* dev_aconns, xyws_accept_result* dev_aresults,
                       const xyws_route_conn* dev_rtconns, uint64_t n,
                       const void* dev_table, uint64_t table_len,
                       xyws_roster_conn* dev_rconns, uint64_t n_rconns,
                       uint32_t default_room, uint32_t policy /* XYWS_RT_MISS_404 */,
                       xyws_route_result* dev_results /* n, nullable */, void* stream);

/* ---- a sweep's send bytes in one buffer ------------------------------------------
 * The last call of a sweep (the reference's chat_session::writer draining
 * m_write_msgs into m_socket.send, and websocket_send_close, once per
 * connection: here for every connection of the sweep at once). The calls before
 * it leave each connection's bytes in its own send range and say how many in a
 * result row; xyws_outbox_streams turns those rows and scattered ranges into
 * three things the host takes with one copy, or reads in place from pinned
 * memory: a dense pack of the send bytes, an ordered send list with one entry
 * per connection that has something to send or must be closed, and a 64-byte
 * summary.
 *
 *  1. Length. For connection i, full_len is the send_len of its backlog row when
 *     one is given, else of its bcast row (a roster row is taken as well: its
 *     first three fields lie alike), else the reply_len of its reply row, else
 *     the resp_len of its accept row when that has XYWS_ACC_ACCEPTED or
 *     XYWS_ACC_REJECTED, else 0: rule 4 of xyws_roster_streams with the backlog
 *     row in front. len = min(full_len, out_cap); out_cap counts as 0 for a null
 *     out.
 *  2. Flags. XYWS_OB_CLOSE: a reply row is given and has XYWS_RPL_CLOSED, or an
 *     accept row is given and has XYWS_ACC_REJECTED. XYWS_OB_OVERFLOW: a reply
 *     row is given and has XYWS_RPL_OVERFLOW. XYWS_OB_TRUNCATED: full_len >
 *     out_cap. XYWS_RPL_CLOSED is sticky: a connection that an earlier sweep
 *     closed is listed with XYWS_OB_CLOSE and len 0 in every sweep until the
 *     caller clears its slot (every row pointer null). A slot with every pointer
 *     null is never listed.
 *  3. The list. Connection i is listed when len > 0 or it has a flag. Entries
 *     are written in ascending i, entry k to entries[k]; entries at and beyond
 *     n_entries are not written. `off` of an entry is the sum of align16(len)
 *     over the listed connections before it.
 *  4. The pack. pack_cap is rounded down to a multiple of 16; a null pack counts
 *     as capacity 0: a plan-only call, whose list and sizes are exact and in
 *     which everything with bytes is deferred. An entry with len > 0 whose slot
 *     [off, off + align16(len)) ends at or below the capacity is packed:
 *     pack[off .. off + len) = out[0 .. len), the remaining bytes of the slot
 *     zero. Otherwise the entry gets XYWS_OB_DEFERRED and no byte of its slot is
 *     written: the caller sends it from `out` itself. Offsets never depend on
 *     the capacity. No byte of the pack outside packed slots is written, and no
 *     destination byte (pack, entries, summary) is read, or written twice: they
 *     may lie across PCIe.
 *  5. Reads. Of `out` only whole 16-byte lines that hold one of out[0 .. len)
 *     are loaded; `out` has any alignment, and neighbours share lines. The rows
 *     and the send ranges are only read, and the call is idempotent: a second
 *     call over the same inputs writes the same bytes.
 *  6. The summary is written once per call, every field exact whatever the
 *     capacity.
 *  7. Properties. Three launches on `stream`: a plan pass, the scan of its tile
 *     sums by one workgroup, and the pack pass; dev_scratch (8-byte aligned,
 *     xyws_outbox_scratch_bytes(n) bytes, the call's alone until the stream has
 *     passed it) is the only hand-over between them. No context scratch, no
 *     atomics, nothing spins; the device error word is untouched, no device
 *     state is read on the host and no reserve is needed: the call can be
 *     captured into a hipGraph at once and runs concurrently on different
 *     streams. n == 0 returns XYWS_OK, launches nothing and leaves the summary
 *     alone. XYWS_ERR_INVALID, decided on the arguments alone, before the
 *     context is used: a null ctx; null dev_conns, entries, summary or
 *     dev_scratch with n > 0; scratch_bytes below xyws_outbox_scratch_bytes(n);
 *     a pack that is not 16-byte aligned; n >= UINT32_MAX.
 *  8. Where the outputs may live. pack, entries and summary are device memory,
 *     or pinned host memory addressed by its device pointer:
 *     xyws_outbox_map(pinned_host, &dev_ptr), called at set-up time, wraps
 *     hipHostGetDevicePointer and returns XYWS_ERR_INVALID with *dev_ptr = NULL
 *     when the memory is not mapped for the device, so that no kernel is ever
 *     handed a host address that was not checked. The host reads such memory
 *     only after the stream has passed the call. */
typedef struct xyws_outbox_conn {     /* 64 bytes; entry i is connection i of the sweep's slot-stable tables */
  const void* out;                    /* device: the connection's send buffer (only read) */
  uint64_t    out_cap;                /* counts as 0 for a null out */
  const xyws_backlog_result* backlog; /* device, nullable: this sweep's rows, as the earlier calls wrote them */
  const xyws_bcast_result*   bcast;   /* ... a roster row is taken as well */
  const xyws_reply_result*   reply;
  const xyws_accept_result*  accept;
  uint64_t    reserved[2];            /* zero */
} xyws_outbox_conn;

typedef struct xyws_outbox_entry {    /* 32 bytes */
  uint32_t conn;      /* table index */
  uint32_t flags;     /* XYWS_OB_* */
  uint64_t off;       /* its slot in the pack: a multiple of 16, exact whatever pack_cap */
  uint64_t len;       /* bytes to send: min(full_len, out_cap) */
  uint64_t full_len;  /* what the sweep produced for it (> len: XYWS_OB_TRUNCATED) */
} xyws_outbox_entry;
#define XYWS_OB_CLOSE     0x1u /* close the socket after these bytes */
#define XYWS_OB_OVERFLOW  0x2u /* reply row has XYWS_RPL_OVERFLOW: the caller closes */
#define XYWS_OB_TRUNCATED 0x4u /* full_len > out_cap: bytes were lost in the send range: the caller closes */
#define XYWS_OB_DEFERRED  0x8u /* its slot does not fit the pack: nothing of it was packed */

typedef struct xyws_outbox_summary {  /* 64 bytes */
  uint64_t n_entries;   /* entries written */
  uint64_t pack_len;    /* sum of all slots, whatever pack_cap */
  uint64_t packed_len;  /* end of the last slot that was packed: the bytes of the pack the host needs */
  uint64_t send_bytes;  /* sum of len */
  uint32_t n_close, n_truncated, n_deferred;
  uint32_t status;      /* XYWS_OBS_* */
  uint64_t reserved[2];
} xyws_outbox_summary;
#define XYWS_OBS_DEFERRED  0x1u /* n_deferred > 0 */
#define XYWS_OBS_TRUNCATED 0x2u /* n_truncated > 0 */

uint64_t xyws_outbox_scratch_bytes(uint64_t n);   /* host; what dev_scratch must hold for n connections */
int xyws_outbox_map(void* pinned_host, void** dev_ptr);
int xyws_outbox_streams(xyws_ctx* ctx, const xyws_outbox_conn* dev_conns, uint64_t n,
                        void* pack, uint64_t pack_cap,
                        xyws_outbox_entry* entries /* room for n */, xyws_outbox_summary* summary,
                        void* dev_scratch, uint64_t scratch_bytes, void* stream);

/* ---- a sweep's received bytes to the connections ----------------------------------
 * The first call of a sweep, the mirror of xyws_outbox_streams (the reference
 * hands every socket its own recv buffer, recv_all.h:86-121; an io_uring
 * service drains its completion queue instead). While it drains, the host
 * fills three things: a dense pack of the received bytes, an entry list with
 * one 32-byte entry per completed recv in arrival order (any number per
 * connection), and a 32-byte head that says how many entries there are.
 * xyws_inbox_streams scatters the bytes into the connections' receive ranges,
 * keeps a small per-connection carry (HTTP, open or dead, and the bytes of an
 * unfinished request) and writes the buf and len words of the slot-stable,
 * resident xyws_conn and xyws_accept_conn rows, so that xyws_accept_streams,
 * xyws_decode_streams and the calls behind them run over tables the host
 * never touches again. The entry count comes from the head, not from an
 * argument: one captured graph serves sweeps of any shape.
 *
 *  1. Entries. M = min(head.m, m_cap); entries from M on are never read
 *     (head.m > m_cap: XYWS_IBM_CLIPPED). With P = min(head.pack_len,
 *     pack_cap) an entry is valid when conn < n and off <= P and
 *     len <= P - off. An entry with conn >= n is ignored and counted in
 *     n_bad_entries; one with conn < n and a bad range is counted there too
 *     and breaks its connection (rule 4). `at` is the host's running count of
 *     the connection's bytes in this sweep before this entry: with it the
 *     order of a connection's bytes does not depend on where its entries
 *     stand in the list.
 *  2. Per connection i, over its valid entries: T = max(at + len), 0 when
 *     there are none; S = the sum of len; eof = any entry of the connection
 *     (bad ranges included) has XYWS_IBE_EOF. n_entries of its result row
 *     counts every entry with conn == i.
 *  3. State step, before anything is placed; s = carry.state.
 *     - s is XYWS_IB_DEAD (or any value above it): the entries are dropped,
 *       XYWS_IBR_DROPPED when there were any, every length written is 0.
 *     - s is HTTP and XYWS_IBC_NO_HANDSHAKE is set: s becomes open (kept and
 *       lead 0, not counted in n_opened).
 *     - s is HTTP and aresult has XYWS_ACC_REJECTED: s becomes dead, the
 *       carry gets the sticky XYWS_IBR_REFUSED, the entries are dropped.
 *     - s is HTTP and aresult has XYWS_ACC_ACCEPTED: the connection opens.
 *       consumed <= http_len is required, otherwise it is broken
 *       (XYWS_IBR_BAD_CONSUMED). kept = http_len - consumed: the frame bytes
 *       that arrived behind the request in an earlier sweep and already lie
 *       in the range. lead = consumed when kept > 0, else 0. The result row
 *       gets XYWS_IBR_OPENED and n_opened counts it, unless rule 4 breaks it.
 *     - otherwise (no aresult, or neither bit) s stays HTTP.
 *     The verdict is the slot's accept row, whoever's request left it:
 *     xyws_accept_streams overwrites it with "incomplete" only in the sweep
 *     after the verdict, when it sees len 0. A slot that changes hands
 *     therefore needs both its carry and its xyws_accept_result row zeroed
 *     before the new connection's first sweep; otherwise the new connection
 *     is refused, or broken by the old `consumed`, on the old one's row.
 *  4. Placement. Base A = http_len while s is HTTP, and in the opening sweep
 *     when kept > 0; otherwise A = 0. The connection is broken when S != T
 *     (XYWS_IBR_BAD_TILING), when A + T > cap (XYWS_IBR_OVERFLOW) or when an
 *     entry of it has a bad range (XYWS_IBR_BAD_RANGE); every bit that
 *     applies is set. Broken: no byte of its range is written, every length
 *     written is 0, lead is 0, the state becomes dead and the bits stay in
 *     the carry until the caller resets it; n_broken counts it. Otherwise
 *     range[A + at, A + at + len) = pack[off, off + len) for every entry.
 *     Entries of one connection that overlap while S == T are the caller's
 *     fault: the bytes inside that connection's own [A, A + T) are then
 *     unspecified, nothing else is touched.
 *  5. Rows. Only the buf and len words are written; carry, frames, cap, out
 *     and out_cap stay the caller's.
 *     - open: conn->buf = buf + lead, conn->len = kept + T (kept only in the
 *       opening sweep), aconn->buf = buf, aconn->len = 0, http_len = 0.
 *     - HTTP: http_len += T; aconn->buf = buf; aconn->len = the new http_len
 *       when T > 0, else 0 (a request that got no new bytes is not parsed
 *       again: xyws_accept_streams reports len 0 as incomplete);
 *       conn->buf = buf, conn->len = 0.
 *     - dead: conn->buf = aconn->buf = buf, both lengths 0; http_len stays.
 *     An idle connection therefore always ends with len 0: no stale length
 *     survives a sweep.
 *  6. EOF. The bytes are still delivered; the result row gets XYWS_IBR_EOF,
 *     and the carry keeps it (a later row shows it again). n_eof counts the
 *     connections whose entries of this sweep had it. Raising the roster's
 *     leave stays with the caller.
 *  7. Outputs. carry.bytes_total grows by the bytes placed. A result row is
 *     written for every i < n: len (bytes placed: T or 0), lead, n_entries,
 *     status (the carry's sticky bits, and XYWS_IBR_DROPPED / XYWS_IBR_OPENED
 *     of this sweep). The summary is written once, every field exact:
 *     n_entries = M, bytes = the sum of len over the rows, n_conns = rows
 *     with n_entries > 0, n_opened, n_eof, n_broken (broken in this sweep),
 *     n_bad_entries, status (XYWS_IBM_*).
 *  8. Memory. No byte outside [buf + A, buf + A + T) of any range is written:
 *     neighbouring ranges share 16-byte lines and have any alignment. Of the
 *     pack only whole 16-byte lines that hold an entry's byte are loaded; off
 *     has any alignment. Head and entries are read by the entry pass only,
 *     which keeps what the later passes need in dev_scratch: in pinned memory
 *     every entry crosses the host link once, and the 32-byte head once per
 *     workgroup of that pass (at most 256 times). The iconn table, head, entries and pack
 *     are only read. The ranges, carries and rows of two entries of dev_iconns
 *     must not overlap.
 *  9. Properties. Five launches on `stream`: clear the per-connection
 *     accumulators; the entry pass (integer atomicAdd / atomicMax / atomicOr
 *     on the accumulators, whose results do not depend on order); the
 *     connection pass, one thread per connection, which also leaves tile
 *     sums; the summary pass of one workgroup; the copy pass, whose grid comes
 *     from m_cap alone, one wave per 1 KiB chunk of an entry. Nothing spins,
 *     no workgroup waits for another. dev_scratch (8-byte aligned,
 *     xyws_inbox_scratch_bytes(n, m_cap) bytes, the call's alone until the
 *     stream has passed it) is the only hand-over. No context scratch; the
 *     device error word is untouched, no device state is read on the host and
 *     no reserve is needed: the call can be captured into a hipGraph at once
 *     and runs concurrently on different streams. n == 0 returns XYWS_OK,
 *     launches nothing and leaves the summary alone. XYWS_ERR_INVALID,
 *     decided on the arguments alone: a null ctx; null dev_iconns, head,
 *     summary or dev_scratch with n > 0; null entries with m_cap > 0; a null
 *     pack with pack_cap > 0; with n > 0 a dev_scratch that is not 8-byte
 *     aligned, or scratch_bytes below xyws_inbox_scratch_bytes(n, m_cap);
 *     n or m_cap >= UINT32_MAX.
 * 10. The invariant. Cut a connection's byte stream (request, then frames)
 *     into entries and sweeps at any points and run xyws_inbox_streams,
 *     xyws_accept_streams, xyws_decode_streams over the slot-stable tables,
 *     sweep after sweep: the accept verdict equals xyws_accept_request on the
 *     request, and the frames, the decoded bytes and the final xyws_carry
 *     equal xyws_decode_stream over the bytes behind `consumed`.
 *
 * Head, entries and pack are device memory, or pinned host memory addressed
 * by the device pointer that xyws_outbox_map returns. */
typedef struct xyws_inbox_head {      /* 32 bytes */
  uint64_t m;          /* entries in the list */
  uint64_t pack_len;   /* bytes of the pack in use */
  uint64_t reserved[2];
} xyws_inbox_head;

typedef struct xyws_inbox_entry {     /* 32 bytes: one completed recv */
  uint32_t conn;       /* table index */
  uint32_t flags;      /* XYWS_IBE_* */
  uint64_t off;        /* in the pack, any alignment */
  uint64_t len;        /* 0 allowed (an EOF alone) */
  uint64_t at;         /* bytes of this connection in this sweep that precede this entry */
} xyws_inbox_entry;
#define XYWS_IBE_EOF 0x1u /* the peer closed behind these bytes */

typedef struct xyws_inbox_carry {     /* 32 bytes; all zero: fresh, HTTP state */
  uint64_t http_len;   /* bytes of the unfinished request in the range */
  uint64_t bytes_total;
  uint32_t state;      /* XYWS_IB_* */
  uint32_t status;     /* the sticky XYWS_IBR_* bits */
  uint64_t reserved;
} xyws_inbox_carry;
#define XYWS_IB_HTTP 0u
#define XYWS_IB_OPEN 1u
#define XYWS_IB_DEAD 2u

typedef struct xyws_inbox_conn {      /* 64 bytes; entry i is connection i of the sweep's slot-stable tables */
  void*                     buf;      /* device: the connection's receive range */
  uint64_t                  cap;
  xyws_inbox_carry*         carry;    /* device; read, then written */
  xyws_conn*                conn;     /* device, nullable: the row whose buf and len are written */
  xyws_accept_conn*         aconn;    /* device, nullable: the row whose buf and len are written */
  const xyws_accept_result* aresult;  /* device, nullable: as the previous sweep left it */
  uint32_t                  flags;    /* XYWS_IBC_* */
  uint32_t                  reserved0;
  uint64_t                  reserved;
} xyws_inbox_conn;
#define XYWS_IBC_NO_HANDSHAKE 0x1u /* the connection never was in HTTP state */

typedef struct xyws_inbox_result {    /* 32 bytes */
  uint64_t len;        /* bytes placed in this sweep */
  uint64_t lead;       /* opening sweep with kept bytes: conn->buf = buf + lead */
  uint32_t n_entries;  /* entries that named this connection */
  uint32_t status;     /* XYWS_IBR_* */
  uint64_t reserved;
} xyws_inbox_result;
#define XYWS_IBR_EOF          0x1u  /* sticky */
#define XYWS_IBR_DROPPED      0x2u  /* this sweep's entries were dropped: the connection is dead */
#define XYWS_IBR_REFUSED      0x4u  /* sticky: its handshake was rejected */
#define XYWS_IBR_BAD_TILING   0x8u  /* sticky: S != T */
#define XYWS_IBR_OVERFLOW     0x10u /* sticky: A + T > cap */
#define XYWS_IBR_BAD_RANGE    0x20u /* sticky: an entry outside the pack */
#define XYWS_IBR_BAD_CONSUMED 0x40u /* sticky: consumed > http_len */
#define XYWS_IBR_OPENED       0x80u /* the connection opened in this sweep */

typedef struct xyws_inbox_summary {   /* 64 bytes */
  uint64_t n_entries;  /* M */
  uint64_t bytes;      /* bytes placed */
  uint32_t n_conns, n_opened, n_eof, n_broken, n_bad_entries;
  uint32_t status;     /* XYWS_IBM_* */
  uint64_t reserved[3];
} xyws_inbox_summary;
#define XYWS_IBM_BAD_ENTRIES 0x1u /* n_bad_entries > 0 */
#define XYWS_IBM_BROKEN      0x2u /* n_broken > 0 */
#define XYWS_IBM_CLIPPED     0x4u /* head.m > m_cap */

uint64_t xyws_inbox_scratch_bytes(uint64_t n, uint64_t m_cap);   /* host */
int xyws_inbox_streams(xyws_ctx* ctx, const xyws_inbox_conn* dev_iconns, uint64_t n,
                       const xyws_inbox_head* head, const xyws_inbox_entry* entries, uint64_t m_cap,
                       const void* pack, uint64_t pack_cap,
                       xyws_inbox_result* dev_results /* n, nullable */, xyws_inbox_summary* summary,
                       void* dev_scratch, uint64_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* XYWS_H */
