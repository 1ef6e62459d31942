// xyws/websocket.hpp — header-only C++20 shim over the xyws C-ABI (xyws.h)
// that keeps the names of xynet's WebSocket frame interface, so a
// websocket.h-style caller switches its decode path by include.
//
//   xynet (reference tree)                               here
//   ---------------------------------------------------  ---------------------------------
//   enum class websocket_flags + operators                xyws::websocket_flags (same values)
//     include/xynet/http/websocket_frame_header.h:42-106
//   detail::calc_frame_header_size / calc_frame_size      xyws::detail::calc_frame_header_size
//     :111-131, WS_MAX_FRAME_HEADER_SIZE :134               / calc_frame_size, WS_MAX_FRAME_HEADER_SIZE
//   websocket_mask(R&& data, uint32_t mask, size_t i)     xyws::websocket_mask(data, mask, i): same
//     include/xynet/http/websocket_frame_mask.h:6-25        signature (host or device bytes, done on
//                                                           return); websocket_mask(ctx, dev span,
//                                                           mask, i, stream): asynchronous, device
//   using namespace xynet (websocket.h:17)                namespace xynet = the names below
//   websocket_frame_header_parser::result()               xyws::frame::result()
//     :264-267 -> tuple<flags, mask_uint32_t, length>
//   websocket_recv_data: parse -> result -> mask          xyws::frame_decoder::decode
//     example/include/common/websocket.h:110-134            (a whole batch of frames per call)
//   class websocket_frame_header :179-224                 xyws::websocket_frame_header (same ctors,
//                                                           view(), span(); masked-ctor quirk kept)
//   class websocket_frame_header_parser :226-385          xyws::websocket_frame_header_parser
//     parse / length / flags / mask_uint32_t / result /     (parsed on the device, xyws_parser_*)
//     mask / reset / npos
//   echo_once reply build (websocket_echo.cpp:18-27)      xyws::encode_frames (batched, device)
//   websocket_check_parser_result (websocket.h:81-108)    xyws::classify_frames (device)
//   (new) FIN=0 chains -> messages, UTF-8 validation      xyws::reassemble (one batch),
//                                                           xyws::message_assembler (across recvs)
//   class websocket_request_handler                       xyws::websocket_request_handler (host: one
//     include/xynet/http/websocket_request_handler.h         request, xyws_accept_request),
//     used by websocket_handshake (websocket.h:40-68)        xyws::accept_streams (many, device)
//
// Nothing but the one-request handshake handler computes on the host: every
// other call goes through libxyws.so to HIP kernels for gfx950. Buffers are caller-owned device memory (hipMalloc);
// `stream` is a hipStream_t passed as void*. Errors throw xyws::error.
#pragma once

#include <array>
#include <concepts>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <ranges>
#include <span>
#include <string_view>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../xyws.h"

namespace xyws {

enum class websocket_flags : unsigned char {
  WS_NONE = 0x0,
  WS_OP_CONTINUE = 0x0,
  WS_OP_TEXT = 0x1,
  WS_OP_BINARY = 0x2,
  WS_OP_CLOSE = 0x8,
  WS_OP_PING = 0x9,
  WS_OP_PONG = 0xA,
  WS_OP_MASK = 0xF,
  WS_FIN = 0x10,
  WS_FINAL_FRAME = 0x10,
  WS_HAS_MASK = 0x20,
};

constexpr websocket_flags operator&(websocket_flags a, websocket_flags b) {
  return websocket_flags(static_cast<unsigned char>(a) & static_cast<unsigned char>(b));
}
constexpr websocket_flags operator|(websocket_flags a, websocket_flags b) {
  return websocket_flags(static_cast<unsigned char>(a) | static_cast<unsigned char>(b));
}
constexpr websocket_flags operator^(websocket_flags a, websocket_flags b) {
  return websocket_flags(static_cast<unsigned char>(a) ^ static_cast<unsigned char>(b));
}
constexpr websocket_flags operator~(websocket_flags a) {
  return websocket_flags(static_cast<unsigned char>(~static_cast<unsigned char>(a)));
}
constexpr websocket_flags& operator&=(websocket_flags& a, websocket_flags b) { return a = a & b; }
constexpr websocket_flags& operator|=(websocket_flags& a, websocket_flags b) { return a = a | b; }
constexpr websocket_flags& operator^=(websocket_flags& a, websocket_flags b) { return a = a ^ b; }
constexpr bool websocket_flags_not_none(websocket_flags f) { return static_cast<unsigned char>(f) != 0; }

namespace detail {
constexpr std::size_t calc_frame_header_size(websocket_flags flags, std::size_t data_len) {
  std::size_t size = 2;
  if (data_len >= 126) size += data_len > 0xFFFF ? 8 : 2;
  if (websocket_flags_not_none(flags & websocket_flags::WS_HAS_MASK)) size += 4;
  return size;
}
constexpr std::size_t calc_frame_size(websocket_flags flags, std::size_t data_len) {
  return data_len + calc_frame_header_size(flags, data_len);
}
}  // namespace detail

inline constexpr std::size_t WS_MAX_FRAME_HEADER_SIZE =
    detail::calc_frame_header_size(websocket_flags::WS_HAS_MASK, 0xFFFFFFFFu);
static_assert(WS_MAX_FRAME_HEADER_SIZE == XYWS_MAX_FRAME_HEADER_SIZE);

class error : public std::runtime_error {
 public:
  error(int code, const char* what)
      : std::runtime_error(std::string(what) + ": " + xyws_strerror(code)), code_(code) {}
  int code() const noexcept { return code_; }

 private:
  int code_;
};

inline void check(int rc, const char* what) {
  if (rc != XYWS_OK) throw error(rc, what);
}

// One context per (thread, device): owns the decoder's device scratch.
class context {
 public:
  explicit context(int device = 0) { check(xyws_ctx_create(device, &h_), "xyws_ctx_create"); }
  ~context() {
    if (h_) xyws_ctx_destroy(h_);
  }
  context(const context&) = delete;
  context& operator=(const context&) = delete;
  context(context&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  context& operator=(context&& o) noexcept {
    if (this != &o) {
      if (h_) xyws_ctx_destroy(h_);
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  // pre-size scratch so later calls allocate nothing (hipGraph capture)
  void reserve(std::uint64_t max_batch_bytes, std::uint64_t max_frames = 0) {
    check(xyws_ctx_reserve(h_, max_batch_bytes, max_frames), "xyws_ctx_reserve");
  }
  std::uint32_t last_device_error() {
    std::uint32_t v = 0;
    check(xyws_ctx_last_device_error(h_, &v), "xyws_ctx_last_device_error");
    return v;
  }
  xyws_ctx* native() const noexcept { return h_; }

 private:
  xyws_ctx* h_ = nullptr;
};

// websocket_mask (websocket_frame_mask.h:6-25) over device bytes: in place,
// data[j] ^= bytes(mask)[(i + j) % 4]; returns i + data.size(). `mask` is
// mask_uint32_t() (the key's wire bytes as a little-endian word).
inline std::size_t websocket_mask(context& ctx, std::span<std::byte> dev_data, std::uint32_t mask,
                                  std::size_t i, void* stream = nullptr) {
  const std::uint8_t key[4] = {std::uint8_t(mask), std::uint8_t(mask >> 8), std::uint8_t(mask >> 16),
                               std::uint8_t(mask >> 24)};
  std::uint64_t out = 0;
  check(xyws_unmask(ctx.native(), dev_data.data(), dev_data.size(), key, i, &out, stream), "xyws_unmask");
  return static_cast<std::size_t>(out);
}

// The calling thread's context on `device` (what default-constructed parsers
// and the reference-signature websocket_mask use, so `websocket_frame_header_parser{}`
// and `websocket_mask(data_span, mask, 0)` read as in the reference).
inline context& default_context(int device = 0) {
  constexpr int MAXDEV = 64;
  thread_local std::array<context*, MAXDEV> ctxs{};
  if (device < 0 || device >= MAXDEV) device = 0;
  if (!ctxs[device]) {
    thread_local struct owner {
      std::array<context*, MAXDEV>* v;
      ~owner() {
        for (auto* c : *v) delete c;
      }
    } own{&ctxs};
    ctxs[device] = new context(device);
  }
  return *ctxs[device];
}

namespace detail {
// websocket_mask's element types (websocket_frame_mask.h:6-13): anything
// convertible to std::byte, char or unsigned char
template <typename T>
inline constexpr bool mask_element_v = std::is_convertible_v<T, std::byte> || std::is_convertible_v<T, char> ||
                                       std::is_convertible_v<T, unsigned char> || std::is_same_v<T, std::byte>;
// a range the device can XOR where it lies: contiguous bytes
template <typename R>
concept contiguous_bytes = std::ranges::contiguous_range<R> && std::ranges::sized_range<R> &&
                           (sizeof(std::ranges::range_value_t<R>) == 1);
// a range of such pieces behind a view (std::views::join over spans: the
// reference's only multi-piece use, test/playground.cpp:188-189)
template <typename R>
concept joined_pieces = requires(R& r) {
  { r.base() } -> std::ranges::range;
} && contiguous_bytes<std::ranges::range_reference_t<decltype(std::declval<R&>().base())>>;

// one contiguous piece (host or device bytes), on the device of its memory
inline std::size_t mask_piece(void* p, std::size_t n, std::uint32_t mask, std::size_t i) {
  if (n == 0) return i;
  const std::uint8_t key[4] = {std::uint8_t(mask), std::uint8_t(mask >> 8), std::uint8_t(mask >> 16),
                               std::uint8_t(mask >> 24)};
  int dev = -1;
  (void)xyws_pointer_device(p, &dev);
  std::uint64_t out = 0;
  check(xyws_mask_bytes(default_context(dev < 0 ? 0 : dev).native(), p, n, key, i, &out, nullptr),
        "xyws_mask_bytes");
  return static_cast<std::size_t>(out);
}
}  // namespace detail

}  // namespace xyws

// websocket_mask(R&& data, uint32_t mask, size_t i) with the reference's
// signature, scope and contract (websocket_frame_mask.h:6-25, declared in the
// global namespace there too): any range of byte-sized elements, host or
// device memory, unmasked in place when it returns, data[j] ^= bytes(mask)[(i
// + j) % 4]; returns i + the range's length. The XOR runs on the device
// through xyws_mask_bytes (host bytes staged: a compatibility path; batches
// go through xyws::frame_decoder):
//  * a contiguous range: one call where it lies;
//  * a view over contiguous pieces (std::views::join of spans, as
//    test/playground.cpp:188-189 masks two joined spans): one call per piece,
//    the phase carried from piece to piece;
//  * any other range: its elements staged in one host buffer, one call,
//    written back in order.
template <typename R>
  requires std::ranges::range<R> && xyws::detail::mask_element_v<std::ranges::range_value_t<R>>
std::size_t websocket_mask(R&& data, std::uint32_t mask, std::size_t i) {
  using namespace xyws::detail;
  if constexpr (contiguous_bytes<R>) {
    return mask_piece(const_cast<void*>(static_cast<const void*>(std::ranges::data(data))), std::ranges::size(data),
                      mask, i);
  } else if constexpr (joined_pieces<std::remove_reference_t<R>>) {
    for (auto&& piece : data.base())
      i = mask_piece(const_cast<void*>(static_cast<const void*>(std::ranges::data(piece))), std::ranges::size(piece),
                     mask, i);
    return i;
  } else {
    std::vector<unsigned char> stage;
    for (auto&& c : data) stage.push_back(static_cast<unsigned char>(c));
    const std::size_t r = mask_piece(stage.data(), stage.size(), mask, i);
    std::size_t j = 0;
    for (auto it = std::ranges::begin(data); it != std::ranges::end(data); ++it, ++j)
      *it = static_cast<std::ranges::range_value_t<R>>(stage[j]);
    return r;
  }
}

namespace xyws {
// (the same function under the shim's namespace: xyws::websocket_mask(data,
// mask, i) and, through namespace xynet below, the reference's spelling)
using ::websocket_mask;

// A decoded frame (device descriptor copied to the host by the caller).
struct frame : xyws_frame {
  websocket_flags flags_() const noexcept { return websocket_flags(xyws_frame::flags); }
  std::uint32_t mask_uint32_t() const noexcept {
    return std::uint32_t(key[0]) | std::uint32_t(key[1]) << 8 | std::uint32_t(key[2]) << 16 |
           std::uint32_t(key[3]) << 24;
  }
  std::size_t length() const noexcept { return static_cast<std::size_t>(payload_len); }
  // websocket_frame_header_parser::result() (:264-267)
  std::tuple<websocket_flags, std::uint32_t, std::size_t> result() const noexcept {
    return {flags_(), mask_uint32_t(), length()};
  }
};
static_assert(sizeof(frame) == sizeof(xyws_frame));

// Batched websocket_recv_data: every frame of each device batch is parsed and
// its payload unmasked in place; a frame or header cut by the batch end
// continues in the next batch through the device-resident carry.
class frame_decoder {
 public:
  // dev_carry: 64 B of caller-owned device memory, zero-filled = fresh stream.
  frame_decoder(context& ctx, xyws_carry* dev_carry, std::uint32_t opts = 0)
      : ctx_(&ctx), carry_(dev_carry), opts_(opts) {}

  // dev_frames (may be empty) receives up to dev_frames.size() descriptors;
  // dev_nframes (nullable device pointer) the frame count.
  void decode(std::span<std::byte> dev_batch, std::span<xyws_frame> dev_frames,
              std::uint64_t* dev_nframes, void* stream = nullptr) {
    check(xyws_decode_stream(ctx_->native(), dev_batch.data(), dev_batch.size(), carry_, carry_,
                             dev_frames.empty() ? nullptr : dev_frames.data(), dev_frames.size(),
                             dev_nframes, opts_, stream),
          "xyws_decode_stream");
  }

  // frames at caller-known offsets (one parser per start, no carry)
  void decode_indexed(std::span<std::byte> dev_batch, const std::uint64_t* dev_starts, std::uint64_t n,
                      xyws_frame* dev_frames, void* stream = nullptr) {
    check(xyws_decode_indexed(ctx_->native(), dev_batch.data(), dev_batch.size(), dev_starts, n, dev_frames,
                              opts_ & XYWS_OPT_PARSE_ONLY, stream),
          "xyws_decode_indexed");
  }

 private:
  context* ctx_;
  xyws_carry* carry_;
  std::uint32_t opts_;
};

// The recv buffers of many connections in one launch (xyws_decode_streams):
// dev_conns is a device table of n xyws_conn entries, each decoded as
// frame_decoder::decode would decode it from its own carry; dev_nframes
// (nullable device pointer, n entries) receives the counts.
inline void decode_streams(context& ctx, const xyws_conn* dev_conns, std::uint64_t n, std::uint64_t* dev_nframes,
                           std::uint32_t opts = 0, void* stream = nullptr) {
  check(xyws_decode_streams(ctx.native(), dev_conns, n, dev_nframes, opts, stream), "xyws_decode_streams");
}

// The answers to what decode_streams found, in one launch (xyws_reply_streams):
// dev_conns and dev_nframes are that call's table and counts, dev_replies[i]
// names connection i's send buffer, reply carry and verdict row. Every frame
// before the connection's first close whose action is in action_mask is echoed
// with `flags` (default: echo_once's FIN | TEXT; with XYWS_ENC_FRAME_OPCODE its
// own opcode, a ping as a pong), a frame cut by the batch end is continued by
// the next call, and a close verdict ends the reply with websocket_send_close's
// frame. dev_results (nullable device pointer, n entries) receives the lengths.
inline void reply_streams(context& ctx, const xyws_conn* dev_conns, const std::uint64_t* dev_nframes,
                          const xyws_reply_conn* dev_replies, std::uint64_t n, std::uint64_t max_payload,
                          std::uint32_t policy = 0,
                          websocket_flags flags = websocket_flags::WS_FINAL_FRAME | websocket_flags::WS_OP_TEXT,
                          std::uint32_t enc_opts = 0, std::uint32_t action_mask = 1u << XYWS_ACT_DATA,
                          xyws_reply_result* dev_results = nullptr, void* stream = nullptr) {
  check(xyws_reply_streams(ctx.native(), dev_conns, dev_nframes, dev_replies, n, max_payload, policy,
                           static_cast<std::uint8_t>(flags), enc_opts, action_mask, dev_results, stream),
        "xyws_reply_streams");
}

// The messages of what decode_streams found, in one launch
// (xyws_reassemble_streams): dev_conns and dev_nframes are that call's table
// and counts, dev_reasm[i] names connection i's message buffer, message carry
// and record row. Each connection is processed as message_assembler::feed
// would process it from its own carry (fragments gathered, text validated,
// a message, frame or UTF-8 sequence cut by the recv boundary continued by the
// next call). Runs before or after reply_streams for the same sweep.
// dev_results (nullable device pointer, n entries) receives lengths and counts.
inline void reassemble_streams(context& ctx, const xyws_conn* dev_conns, const std::uint64_t* dev_nframes,
                               const xyws_reasm_conn* dev_reasm, std::uint64_t n,
                               std::uint32_t opts = XYWS_REASM_UTF8, xyws_reasm_result* dev_results = nullptr,
                               void* stream = nullptr) {
  check(xyws_reassemble_streams(ctx.native(), dev_conns, dev_nframes, dev_reasm, n, opts, dev_results, stream),
        "xyws_reassemble_streams");
}

// The room of the same sweep, in at most two launches (xyws_broadcast_streams):
// dev_reasm and dev_reasm_results are the table and the rows of the
// reassemble_streams call, dev_bconns[i] names connection i's message head,
// send buffer, reply result row (nullable) and room. Every room's whole
// messages are framed once with `flags` (default: the chat writer's
// FIN | TEXT; with XYWS_ENC_FRAME_OPCODE each message's own opcode) into the
// room's wire, and the wire is appended to every member's send range behind
// its reply. dev_room_results (n_rooms entries) is required with n_rooms > 0;
// dev_results (nullable device pointer, n entries) receives the send lengths.
inline void broadcast_streams(context& ctx, const xyws_reasm_conn* dev_reasm,
                              const xyws_reasm_result* dev_reasm_results, const xyws_bcast_conn* dev_bconns,
                              std::uint64_t n, const xyws_room* dev_rooms, xyws_room_result* dev_room_results,
                              std::uint64_t n_rooms,
                              websocket_flags flags = websocket_flags::WS_FINAL_FRAME | websocket_flags::WS_OP_TEXT,
                              std::uint32_t enc_opts = 0, xyws_bcast_result* dev_results = nullptr,
                              void* stream = nullptr) {
  check(xyws_broadcast_streams(ctx.native(), dev_reasm, dev_reasm_results, dev_bconns, n, dev_rooms,
                               dev_room_results, n_rooms, static_cast<std::uint8_t>(flags), enc_opts, dev_results,
                               stream),
        "xyws_broadcast_streams");
}

// The messages a recv boundary cut, between reassemble_streams and
// broadcast_streams of the same sweep, in one launch (xyws_hold_streams):
// dev_hold[i] names connection i's hold (the hold_cap bytes in front of its
// reassembly range), its hold carry and the view's record row. The call keeps
// the parts of an open message in the hold and writes dev_view and
// dev_view_results (n entries each), which broadcast_streams takes in place of
// dev_reasm and dev_reasm_results: in the sweep that completes a held message
// the view names it as one whole record. dev_results (nullable device pointer,
// n entries) receives what was held, delivered or lost.
inline void hold_streams(context& ctx, const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                         const xyws_hold_conn* dev_hold, std::uint64_t n, xyws_reasm_conn* dev_view,
                         xyws_reasm_result* dev_view_results, xyws_hold_result* dev_results = nullptr,
                         void* stream = nullptr) {
  check(xyws_hold_streams(ctx.native(), dev_reasm, dev_reasm_results, dev_hold, n, dev_view, dev_view_results,
                          dev_results, stream),
        "xyws_hold_streams");
}

// The room's recent messages, after broadcast_streams of the same sweep, in at
// most two launches (xyws_backlog_streams; the reference's m_recent_messages
// and deliver_recent_messages): the first seven table arguments are the ones
// broadcast_streams was given plus the room rows it wrote. dev_brooms[r] names
// room r's log, its carry and how many frames to keep: the sweep's newest
// frames are folded into the log. dev_jconns[i] (nullable table: fold only)
// names connection i's send buffer, its broadcast and reply rows and, with
// XYWS_BL_JOIN, the room it joins: the room's backlog is appended behind its
// send bytes. A joiner becomes a member of its room from the next sweep on.
// dev_broom_results (n_rooms entries) and dev_results (n entries) are nullable.
inline void backlog_streams(context& ctx, const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                            const xyws_bcast_conn* dev_bconns, std::uint64_t n, const xyws_room* dev_rooms,
                            const xyws_room_result* dev_room_results, const xyws_backlog_room* dev_brooms,
                            xyws_backlog_room_result* dev_broom_results, std::uint64_t n_rooms,
                            const xyws_backlog_conn* dev_jconns = nullptr, xyws_backlog_result* dev_results = nullptr,
                            void* stream = nullptr) {
  check(xyws_backlog_streams(ctx.native(), dev_reasm, dev_reasm_results, dev_bconns, n, dev_rooms, dev_room_results,
                             dev_brooms, dev_broom_results, n_rooms, dev_jconns, dev_results, stream),
        "xyws_backlog_streams");
}

// Who is in the room, between broadcast_streams and backlog_streams of the same
// sweep, in at most three launches (xyws_roster_streams; the reference's
// m_participants, join, leave, welcome and farewell). dev_bconns and dev_rooms
// are the broadcast's tables, resident on the device: the member lists, their
// counts and each connection's room are rewritten here for the next sweep.
// dev_rconns[i] names connection i's address text, its send buffer, this
// sweep's broadcast, reply and accept rows and what it asks (XYWS_RS_*);
// dev_rrooms[r] the capacity of room r's member array, its notice wire and its
// `seen` row, which receives the list as the broadcast read it: this sweep's
// backlog_streams is given the seen rows in place of dev_rooms.
// The leavers' farewells and the joiners' welcomes are framed with `flags`
// and appended behind every participant's send bytes. dev_jconns (nullable)
// is the backlog call's table: the joiners are marked in it. text (host,
// nullable) replaces the reference's three strings.
inline void roster_streams(context& ctx, xyws_bcast_conn* dev_bconns, const xyws_roster_conn* dev_rconns,
                           std::uint64_t n, xyws_room* dev_rooms, const xyws_roster_room* dev_rrooms,
                           xyws_roster_room_result* dev_room_results, std::uint64_t n_rooms, std::uint32_t* dev_want,
                           xyws_roster_result* dev_results, xyws_backlog_conn* dev_jconns = nullptr,
                           std::uint8_t flags = XYWS_FLAG_FIN | XYWS_FLAG_OP_TEXT, const xyws_roster_text* text = nullptr,
                           void* stream = nullptr) {
  check(xyws_roster_streams(ctx.native(), dev_bconns, dev_rconns, n, dev_rooms, dev_rrooms, dev_room_results, n_rooms,
                            text, flags, dev_jconns, dev_want, dev_results, stream),
        "xyws_roster_streams");
}

// The opening handshakes of the connections still in HTTP state, in one launch
// (xyws_accept_streams), before any of the calls above sees them: dev_conns[i]
// names every byte connection i has sent so far and its send buffer. A whole
// request is checked (RFC 6455 4.2.1, or the reference's handler under
// XYWS_ACC_REFERENCE) and answered with the 101, a 400 or a 426; an incomplete
// one is reported as incomplete and nothing is written. dev_results (nullable
// device pointer, n entries) receives the verdicts; on ACCEPTED the bytes
// behind `consumed` are the connection's first frame bytes.
inline void accept_streams(context& ctx, const xyws_accept_conn* dev_conns, std::uint64_t n,
                           xyws_accept_result* dev_results = nullptr, std::uint32_t policy = 0,
                           std::uint32_t max_request = 1024, void* stream = nullptr) {
  check(xyws_accept_streams(ctx.native(), dev_conns, n, max_request, policy, dev_results, stream),
        "xyws_accept_streams");
}

// The route table of xyws_route_streams, built on the host (xyws_route_build):
// one opaque blob, to be copied to 4-byte-aligned device memory as it is.
// slots = 0 lets the library choose the table's size. Throws xyws::error for
// what the build refuses (an empty or too long key, `?` or `#` in a key, two
// keys equal once a trailing `/` is dropped, unknown flags, a bad slot count).
inline std::vector<std::byte> route_table(std::span<const xyws_route> routes, std::uint32_t slots = 0) {
  std::uint64_t need = 0;
  const int rc = xyws_route_build(routes.data(), static_cast<std::uint32_t>(routes.size()), slots, nullptr, 0, &need);
  if (rc != XYWS_ERR_CAPACITY) check(rc ? rc : XYWS_ERR_INVALID, "xyws_route_build");
  std::vector<std::byte> blob(need);
  check(xyws_route_build(routes.data(), static_cast<std::uint32_t>(routes.size()), slots, blob.data(), need, &need),
        "xyws_route_build");
  return blob;
}

// Which room every accepted connection goes to, in one launch between
// accept_streams and roster_streams (xyws_route_streams): the request target of
// dev_aconns[k] / dev_aresults[k] is looked up in the device copy of a
// route_table() blob and the room is stored into dev_rconns[dev_rtconns[k].rconn],
// which XYWS_RS_JOIN_ON_ACCEPT then joins. A target no route matches goes to
// default_room (XYWS_ROOM_NONE: accepted, in no room) or, under
// XYWS_RT_MISS_404, gets `404 Not Found` over its 101 and a rejected accept
// row. dev_results (nullable device pointer, n entries) receives the route rows.
inline void route_streams(context& ctx, const xyws_accept_conn* dev_aconns, xyws_accept_result* dev_aresults,
                          const xyws_route_conn* dev_rtconns, std::uint64_t n, const void* dev_table,
                          std::uint64_t table_len, xyws_roster_conn* dev_rconns, std::uint64_t n_rconns,
                          xyws_route_result* dev_results = nullptr, std::uint32_t default_room = XYWS_ROOM_NONE,
                          std::uint32_t policy = 0, void* stream = nullptr) {
  check(xyws_route_streams(ctx.native(), dev_aconns, dev_aresults, dev_rtconns, n, dev_table, table_len, dev_rconns,
                           n_rconns, default_room, policy, dev_results, stream),
        "xyws_route_streams");
}

// What a sweep left to send, packed into one buffer by its last call
// (xyws_outbox_streams, three launches): dev_conns[i] names connection i's send
// buffer and the rows the sweep's calls wrote for it. `pack` (16-byte aligned,
// pack_cap bytes; null: a plan-only call) receives the send bytes in slots that
// begin at multiples of 16, `entries` (room for n) one entry per connection
// that sends or must be closed, in table order, `summary` the counts and
// sizes. The three may be device memory or pinned host memory addressed by its
// device pointer (outbox_map). dev_scratch: outbox_scratch_bytes(n) bytes of
// device memory, the call's own until the stream has passed it.
inline std::uint64_t outbox_scratch_bytes(std::uint64_t n) { return xyws_outbox_scratch_bytes(n); }
inline void outbox_streams(context& ctx, const xyws_outbox_conn* dev_conns, std::uint64_t n, void* pack,
                           std::uint64_t pack_cap, xyws_outbox_entry* entries, xyws_outbox_summary* summary,
                           void* dev_scratch, std::uint64_t scratch_bytes, void* stream = nullptr) {
  check(xyws_outbox_streams(ctx.native(), dev_conns, n, pack, pack_cap, entries, summary, dev_scratch, scratch_bytes,
                            stream),
        "xyws_outbox_streams");
}
// The device pointer of pinned host memory for outbox_streams' outputs, checked
// once at set-up time. Throws xyws::error when the memory is not mapped for the
// device.
inline void* outbox_map(void* pinned_host) {
  void* dev = nullptr;
  check(xyws_outbox_map(pinned_host, &dev), "xyws_outbox_map");
  return dev;
}

// A sweep's received bytes scattered to the connections by its first call
// (xyws_inbox_streams, five launches): dev_iconns[i] names connection i's
// receive range, its inbox carry and the resident xyws_conn and
// xyws_accept_conn rows whose buf and len the call writes. `head` says how
// many of the `entries` (room for m_cap) the sweep brought, `pack` (pack_cap
// bytes) holds their bytes; the three may be device memory or pinned host
// memory addressed by its device pointer (outbox_map). dev_results (n rows,
// nullable) and `summary` receive what was placed. dev_scratch:
// inbox_scratch_bytes(n, m_cap) bytes of device memory, the call's own until
// the stream has passed it.
inline std::uint64_t inbox_scratch_bytes(std::uint64_t n, std::uint64_t m_cap) {
  return xyws_inbox_scratch_bytes(n, m_cap);
}
inline void inbox_streams(context& ctx, const xyws_inbox_conn* dev_iconns, std::uint64_t n, const xyws_inbox_head* head,
                          const xyws_inbox_entry* entries, std::uint64_t m_cap, const void* pack, std::uint64_t pack_cap,
                          xyws_inbox_result* dev_results, xyws_inbox_summary* summary, void* dev_scratch,
                          std::uint64_t scratch_bytes, void* stream = nullptr) {
  check(xyws_inbox_streams(ctx.native(), dev_iconns, n, head, entries, m_cap, pack, pack_cap, dev_results, summary,
                           dev_scratch, scratch_bytes, stream),
        "xyws_inbox_streams");
}

// class websocket_request_handler (websocket_request_handler.h:66-264) over
// xyws_accept_request: host memory only, no context, no device. parse() takes
// the accumulated request and returns what the reference's does: the bytes
// consumed, -1 for a grammar error, -2 while incomplete. generate_response()
// returns the 101 or, as there, the bad-request response for whatever was not
// a whole valid request (an incomplete one included). The default policy is
// the reference's (XYWS_ACC_REFERENCE); policy 0 answers by RFC 6455 4.2.1.
// get_path() views the caller's bytes, as in the reference.
class websocket_request_handler {
 public:
  explicit websocket_request_handler(std::uint32_t policy = XYWS_ACC_REFERENCE,
                                     std::uint32_t max_request = XYWS_ACCEPT_MAX_REQUEST)
      : policy_(policy), max_request_(max_request) {}

  int parse(std::string_view str) { return parse(str.data(), str.size()); }
  template <typename T, std::size_t Extent>
  int parse(std::span<T, Extent> span) {
    const auto bytes = std::as_bytes(span);
    return parse(reinterpret_cast<const char*>(bytes.data()), bytes.size());
  }

  std::span<const std::byte> generate_response() {
    if (!(res_.status & XYWS_ACC_ACCEPTED) && !(res_.status & XYWS_ACC_REJECTED)) {
      // not parsed (never, or incomplete): the handler's bad request, as in the reference
      xyws_accept_result r{};
      static constexpr char bad[] = "\x01";
      check(xyws_accept_request(bad, 1, max_request_, policy_, response_.data(), response_.size(), &r),
            "xyws_accept_request");
      resp_len_ = r.resp_len;
    }
    return response();
  }
  std::span<const std::byte> response() const {
    return {reinterpret_cast<const std::byte*>(response_.data()), resp_len_};
  }
  std::string_view response_view() const { return {response_.data(), resp_len_}; }
  std::span<const std::byte> bad_request_response() const {
    static constexpr char bad[] = "HTTP/1.1 400 Bad Request\r\n";
    return {reinterpret_cast<const std::byte*>(bad), sizeof(bad) - 1};
  }
  std::string_view get_path() const { return {req_ + res_.path_off, res_.path_len}; }
  bool accepted() const { return (res_.status & XYWS_ACC_ACCEPTED) != 0; }
  const xyws_accept_result& result() const { return res_; }

 private:
  int parse(const char* p, std::size_t n) {
    req_ = p;
    res_ = xyws_accept_result{};
    check(xyws_accept_request(p, n, max_request_, policy_, response_.data(), response_.size(), &res_),
          "xyws_accept_request");
    resp_len_ = res_.resp_len;
    if (res_.reason == XYWS_ACR_PARSE) return -1;
    if (!res_.consumed) return -2;  // incomplete, or longer than max_request without an end
    return static_cast<int>(res_.consumed);
  }

  std::uint32_t policy_, max_request_;
  const char* req_ = "";
  xyws_accept_result res_{};
  std::array<char, 144> response_{};
  std::size_t resp_len_ = 0;
};

// class websocket_frame_header (websocket_frame_header.h:179-224): a header in
// a 14-byte array. As in the reference, the masked constructors keep the key
// beside the header and build it with the key bytes zero (:183-202); with_key()
// builds the RFC client-role header that carries the key.
class websocket_frame_header {
 public:
  websocket_frame_header(websocket_flags flags, std::size_t data_len) noexcept {
    len_ = static_cast<std::size_t>(
        xyws_header_build(static_cast<std::uint8_t>(flags), nullptr, data_len, hdr_.data()));
  }
  websocket_frame_header(websocket_flags flags, std::span<char, 4> mask, std::size_t data_len) noexcept
      : websocket_frame_header{flags, data_len} {
    std::memcpy(mask_.data(), mask.data(), 4);
  }
  websocket_frame_header(websocket_flags flags, std::uint32_t mask, std::size_t data_len) noexcept
      : websocket_frame_header{flags, data_len} {
    std::memcpy(mask_.data(), &mask, 4);
  }
  static websocket_frame_header with_key(websocket_flags flags, std::uint32_t key, std::size_t data_len) noexcept {
    websocket_frame_header h{flags | websocket_flags::WS_HAS_MASK, data_len};
    std::uint8_t k[4];
    std::memcpy(k, &key, 4);
    h.len_ = static_cast<std::size_t>(xyws_header_build(
        static_cast<std::uint8_t>(flags | websocket_flags::WS_HAS_MASK), k, data_len, h.hdr_.data()));
    std::memcpy(h.mask_.data(), &key, 4);
    return h;
  }
  [[nodiscard]] std::string_view view() const {
    return {reinterpret_cast<const char*>(hdr_.data()), len_};
  }
  [[nodiscard]] std::span<const std::byte> span() const {
    return {reinterpret_cast<const std::byte*>(hdr_.data()), len_};
  }

 private:
  std::array<std::uint8_t, XYWS_MAX_FRAME_HEADER_SIZE> hdr_ = {};
  std::array<char, 4> mask_ = {};
  std::size_t len_ = 0;
};

// class websocket_frame_header_parser (websocket_frame_header.h:226-385). parse()
// takes host or device bytes and returns the bytes consumed in this call up to
// the end of the header, or npos while it is incomplete; after a complete
// header it returns npos until reset(). The parse runs on the device (the
// stream decoder in parse-only mode, device-resident carry); it is synchronous
// on `stream`. Unlike the reference it can throw xyws::error (a HIP failure).
class websocket_frame_header_parser {
 public:
  static constexpr std::size_t npos = static_cast<std::size_t>(-1);

  websocket_frame_header_parser() : websocket_frame_header_parser(default_context()) {}
  explicit websocket_frame_header_parser(context& ctx, void* stream = nullptr) : stream_(stream) {
    check(xyws_parser_create(ctx.native(), &p_), "xyws_parser_create");
  }
  ~websocket_frame_header_parser() {
    if (p_) xyws_parser_destroy(p_);
  }
  websocket_frame_header_parser(const websocket_frame_header_parser&) = delete;
  websocket_frame_header_parser& operator=(const websocket_frame_header_parser&) = delete;
  websocket_frame_header_parser(websocket_frame_header_parser&& o) noexcept
      : p_(std::exchange(o.p_, nullptr)), stream_(o.stream_) {}

  std::size_t parse(std::string_view str) { return parse_bytes(str.data(), str.size()); }
  template <typename T, std::size_t Extent>
  std::size_t parse(std::span<T, Extent> sp) {
    const auto b = std::as_bytes(sp);
    return parse_bytes(b.data(), b.size());
  }

  std::size_t length() const noexcept { return static_cast<std::size_t>(get().payload_len); }
  websocket_flags flags() const noexcept { return websocket_flags(get().flags); }
  std::uint32_t mask_uint32_t() const noexcept {
    const xyws_frame f = get();
    std::uint32_t m;
    std::memcpy(&m, f.key, 4);  // wire bytes reinterpreted as a host int (:259-262)
    return m;
  }
  std::tuple<websocket_flags, std::uint32_t, std::size_t> result() const noexcept {
    return {flags(), mask_uint32_t(), length()};
  }
  std::array<char, 4> mask() const noexcept {
    const xyws_frame f = get();
    std::array<char, 4> m;
    std::memcpy(m.data(), f.key, 4);
    return m;
  }
  void reset() { check(xyws_parser_reset(p_), "xyws_parser_reset"); }

 private:
  std::size_t parse_bytes(const void* data, std::size_t len) {
    std::uint64_t consumed = XYWS_NPOS;
    check(xyws_parser_parse(p_, data, len, &consumed, stream_), "xyws_parser_parse");
    return consumed == XYWS_NPOS ? npos : static_cast<std::size_t>(consumed);
  }
  xyws_frame get() const noexcept {
    xyws_frame f{};
    std::uint64_t len = 0;
    (void)xyws_parser_result(p_, &f.flags, f.key, &len);
    f.payload_len = len;
    return f;
  }

  xyws_parser* p_ = nullptr;
  void* stream_ = nullptr;
};

// Batched echo replies / client-role frames on the device (xyws_encode_frames).
inline void encode_frames(context& ctx, std::span<const std::byte> dev_src, std::span<const xyws_frame> dev_frames,
                          const std::uint64_t* dev_n, websocket_flags flags, std::span<std::byte> dev_out,
                          std::uint64_t* dev_out_len, std::uint32_t enc_opts = 0,
                          const std::uint8_t* dev_keys = nullptr, const xyws_verdict* dev_verdicts = nullptr,
                          std::uint32_t action_mask = 0, std::uint64_t* dev_offsets = nullptr,
                          void* stream = nullptr) {
  check(xyws_encode_frames(ctx.native(), dev_src.data(), dev_src.size(), dev_frames.data(), dev_frames.size(), dev_n,
                           static_cast<std::uint8_t>(flags), enc_opts, dev_keys, dev_verdicts, action_mask,
                           dev_out.data(), dev_out.size(), dev_offsets, dev_out_len, stream),
        "xyws_encode_frames");
}

// websocket_check_parser_result's policy per frame (xyws_classify_frames).
inline void classify_frames(context& ctx, std::span<const std::byte> dev_src, std::span<const xyws_frame> dev_frames,
                            const std::uint64_t* dev_n, std::uint64_t max_payload, std::uint32_t policy,
                            xyws_verdict* dev_verdicts, std::uint64_t* dev_first_close, void* stream = nullptr) {
  check(xyws_classify_frames(ctx.native(), dev_src.data(), dev_src.size(), dev_frames.data(), dev_frames.size(),
                             dev_n, max_payload, policy, dev_verdicts, dev_first_close, stream),
        "xyws_classify_frames");
}

// FIN=0 chains of one batch gathered into messages, with UTF-8 validation
// under XYWS_REASM_UTF8 (xyws_reassemble): dev_out receives the payloads back
// to back, dev_msgs the records, *dev_nmsgs (nullable) their count.
inline void reassemble(context& ctx, std::span<const std::byte> dev_src, std::span<const xyws_frame> dev_frames,
                       const std::uint64_t* dev_n, std::uint32_t opts, std::span<std::byte> dev_out,
                       std::span<xyws_message> dev_msgs, std::uint64_t* dev_nmsgs, void* stream = nullptr) {
  check(xyws_reassemble(ctx.native(), dev_src.data(), dev_src.size(), dev_frames.data(), dev_frames.size(), dev_n,
                        opts, dev_out.data(), dev_out.size(), dev_msgs.data(), dev_msgs.size(), dev_nmsgs, stream),
        "xyws_reassemble");
}

// Reassembly across batch boundaries (xyws_reassemble_stream): feed() takes
// each batch frame_decoder::decode decoded, with that call's frame table, in
// order; a message, a frame or a UTF-8 sequence cut by the batch end continues
// in the next batch through the device-resident carry. Record 0 of a call is
// the continuation of the message the last one left open (XYWS_MSG_CONTINUED).
class message_assembler {
 public:
  // dev_carry: 64 B of caller-owned device memory, zero-filled = fresh stream.
  message_assembler(context& ctx, xyws_msg_carry* dev_carry, std::uint32_t opts = XYWS_REASM_UTF8)
      : ctx_(&ctx), carry_(dev_carry), opts_(opts) {}

  void feed(std::span<const std::byte> dev_batch, std::span<const xyws_frame> dev_frames, const std::uint64_t* dev_n,
            std::span<std::byte> dev_out, std::span<xyws_message> dev_msgs, std::uint64_t* dev_nmsgs,
            void* stream = nullptr) {
    check(xyws_reassemble_stream(ctx_->native(), dev_batch.data(), dev_batch.size(), dev_frames.data(),
                                 dev_frames.size(), dev_n, opts_, carry_, carry_, dev_out.data(), dev_out.size(),
                                 dev_msgs.data(), dev_msgs.size(), dev_nmsgs, stream),
          "xyws_reassemble_stream");
  }

 private:
  context* ctx_;
  xyws_msg_carry* carry_;
  std::uint32_t opts_;
};

}  // namespace xyws

// The reference's namespace (websocket_frame_header.h, `using namespace xynet`
// at example/include/common/websocket.h:17): its frame names resolve to the
// ones above, so a caller switches by include.
namespace xynet {
using namespace ::xyws;
}
