"""Host-side mirror of xynet's WebSocket frame interface, backed by the gfx950 path.

Names, argument meaning and error behaviour follow the reference headers
(paths relative to the xynet tree):

  websocket_flags                  include/xynet/http/websocket_frame_header.h:42-106
  calc_frame_header_size / _size   :111-131, WS_MAX_FRAME_HEADER_SIZE :134
  websocket_frame_header           :179-224  (xyws_header_build, the reference builder's
                                              bytes; one header, no device work)
  websocket_frame_header_parser    :226-385  (xyws_parser_*: parsed on the device)
  websocket_mask                   include/xynet/http/websocket_frame_mask.h:6-25
  frame_decoder.decode             the batched websocket_recv_data
                                   (example/include/common/websocket.h:110-134)
  connection_group.decode          the same for many connections at once, one launch
                                   (xyws_decode_streams: one coroutine's loop per wave)
  connection_group.reply           the rest of that loop for many connections at once: close policy,
                                   echo_once, websocket_send_close (xyws_reply_streams, one launch)
  connection_group.accept          websocket_handshake (example/include/common/websocket.h:40-68) for many
                                   connections at once: the HTTP upgrade parsed, checked and answered
                                   (xyws_accept_streams, one launch)
  connection_group.rooms / roster  chat_room's participants, join, leave, welcome and farewell
                                   (example/websocket/websocket_chat.cpp:34-39, 49-87) for many rooms at
                                   once, the lists kept on the device (xyws_roster_streams)
  websocket_request_handler       include/xynet/http/websocket_request_handler.h:66-264, one request on
                                   the host (xyws_accept_request: the kernel's grammar compiled for the host)
  encode_frames                    echo_once's replies, batched on the device
                                   (example/websocket/websocket_echo.cpp:18-27)
  classify_frames                  websocket_check_parser_result's policy
                                   (example/include/common/websocket.h:81-108)
  reassemble                       FIN=0 chains -> messages (+ UTF-8 check)
  message_assembler.feed           the same across recv boundaries (xyws_reassemble_stream)
  shard_plan / shard_plan_frames   one batch cut at frame boundaries across devices
                                   (a host-side header walk)

Device buffers are torch uint8 tensors on a ROCm device (PyTorch is used only
for device memory and streams). Every computing call runs HIP kernels from
libxyws.so through its C-ABI; there is no CPU fallback. The one host-only
class is websocket_request_handler: one handshake request in host memory, by
design (the batched path is connection_group.accept, on the device).
"""
import ctypes as C
import enum
import threading

from . import _lib
from ._lib import XYWS_OK, Carry, Frame, XywsError, check

npos = (1 << 64) - 1


class websocket_flags(enum.IntFlag):
    """enum class websocket_flags (websocket_frame_header.h:42-58)."""
    WS_NONE = 0x0
    WS_OP_CONTINUE = 0x0
    WS_OP_TEXT = 0x1
    WS_OP_BINARY = 0x2
    WS_OP_CLOSE = 0x8
    WS_OP_PING = 0x9
    WS_OP_PONG = 0xA
    WS_OP_MASK = 0xF
    WS_FIN = 0x10
    WS_FINAL_FRAME = 0x10
    WS_HAS_MASK = 0x20


def websocket_flags_not_none(flag):
    """websocket_flags_not_none (:61-64)."""
    return bool(int(flag))


def calc_frame_header_size(flags, data_len):
    """detail::calc_frame_header_size (:111-126)."""
    size = 2
    if data_len >= 126:
        size += 8 if data_len > 0xFFFF else 2
    if int(flags) & websocket_flags.WS_HAS_MASK:
        size += 4
    return size


def calc_frame_size(flags, data_len):
    """detail::calc_frame_size (:128-131)."""
    return data_len + calc_frame_header_size(flags, data_len)


WS_MAX_FRAME_HEADER_SIZE = calc_frame_header_size(websocket_flags.WS_HAS_MASK, 0xFFFFFFFF)


def _builder(flags, mask, data_len):
    """detail::websocket_frame_header_builder (:136-175) through xyws_header_build:
    the header bytes; key bytes are written only when `mask` is given (:168-171)."""
    L = _lib.load()
    out = (C.c_uint8 * 16)()
    key = None if mask is None else (C.c_uint8 * 4)(*bytes(mask))
    n = L.xyws_header_build(int(flags) & 0xFF, key, int(data_len) & ((1 << 64) - 1), out)
    return bytes(out[:n])


class websocket_frame_header:
    """class websocket_frame_header (:179-224).

    Reference behaviour is kept in parity mode: the masked constructors store
    the key beside the header and build the header WITHOUT it (:186-188,
    :191-202), so the key bytes on the wire are zero. ``with_key`` builds the
    RFC-correct masked header (client role) instead.
    """

    def __init__(self, flags, data_len, mask=None):
        self._mask = b"\0\0\0\0"
        if mask is not None:
            self._mask = (mask.to_bytes(4, "little") if isinstance(mask, int) else bytes(mask))
        self._header = _builder(flags, None, data_len)

    @classmethod
    def with_key(cls, flags, data_len, key):
        h = cls(flags, data_len)
        key = key.to_bytes(4, "little") if isinstance(key, int) else bytes(key)
        h._mask = key
        h._header = _builder(int(flags) | websocket_flags.WS_HAS_MASK, key, data_len)
        return h

    def view(self):
        return self._header

    def span(self):
        return self._header

    def __len__(self):
        return len(self._header)


# ---------------------------------------------------------------------------
# device plumbing

class Context:
    """An xyws_ctx bound to one HIP device (one per thread and device)."""

    def __init__(self, device=0):
        self.L = _lib.load()
        self.device = device
        h = C.c_void_p()
        check(self.L.xyws_ctx_create(device, C.byref(h)), "xyws_ctx_create")
        self.h = h

    def reserve(self, max_batch_bytes, max_frames=0):
        check(self.L.xyws_ctx_reserve(self.h, max_batch_bytes, max_frames), "xyws_ctx_reserve")

    def reserve_iov(self, max_total_bytes):
        """xyws_ctx_reserve_iov: the buffer-sequence decode's staging buffer."""
        check(self.L.xyws_ctx_reserve_iov(self.h, max_total_bytes), "xyws_ctx_reserve_iov")

    def last_device_error(self):
        """Device error word of the calls since the last read (0 = none);
        synchronizes the device and clears the word (xyws.h)."""
        v = C.c_uint32()
        rc = self.L.xyws_ctx_last_device_error(self.h, C.byref(v))
        if rc not in (XYWS_OK, _lib.XYWS_ERR_DEVICE):
            check(rc, "xyws_ctx_last_device_error")
        return v.value

    def close(self):
        if getattr(self, "h", None):
            self.L.xyws_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_tls = threading.local()


def context(device=None):
    import torch
    dev = torch.cuda.current_device() if device is None else int(device)
    cache = getattr(_tls, "ctx", None)
    if cache is None:
        cache = _tls.ctx = {}
    if dev not in cache:
        cache[dev] = Context(dev)
    return cache[dev]


def _dev_u8(t):
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise XywsError(-1, "expected a device-resident torch tensor")
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise XywsError(-1, "expected a contiguous uint8 tensor")
    return t


def _stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def websocket_mask(data, mask, i=0):
    """websocket_mask(R&& data, uint32_t mask, size_t i) -> size_t
    (websocket_frame_mask.h:6-25) on a device tensor: in place,
    data[j] ^= bytes(mask)[(i + j) % 4]; returns i + len(data)."""
    t = _dev_u8(data)
    ctx = context(t.device.index)
    key = (C.c_uint8 * 4)(*int(mask & 0xFFFFFFFF).to_bytes(4, "little"))
    out = C.c_uint64()
    check(ctx.L.xyws_unmask(ctx.h, C.c_void_p(t.data_ptr()), t.numel(), key, int(i),
                            C.byref(out), _stream(t)), "xyws_unmask")
    return out.value


class _Rows:
    """The first n rows (ctypes structure `struct`) of a device uint8 tensor
    as host copies: the tensor is copied once, when a row is first asked for;
    an index outside the call's items is an IndexError."""

    def __init__(self, struct, t, n):
        self.struct, self.t, self.n, self._raw = struct, t, n, None

    def __getitem__(self, k):
        if not 0 <= k < self.n:
            raise IndexError(k)
        size = C.sizeof(self.struct)
        if self._raw is None:
            self._raw = self.t[:size * max(self.n, 1)].cpu().numpy().tobytes()
        return self.struct.from_buffer_copy(self._raw, size * k)


class DecodeResult:
    """Frames and count of one decode call (device tensors; host copies on demand)."""

    def __init__(self, frames_t, nframes_t, cap):
        self.frames_t = frames_t
        self.nframes_t = nframes_t
        self.cap = cap

    @property
    def nframes(self):
        return int(self.nframes_t.item()) if self.nframes_t is not None else None

    def frames(self):
        if self.frames_t is None:
            return []
        return _lib.read_rows(Frame, self.frames_t, min(self.nframes, self.cap))


class frame_decoder:
    """Batched, device-resident websocket_recv_data: parse every frame of
    back-to-back batches and unmask payloads in place, carrying a frame or header
    cut by a batch end into the next batch (xyws_decode_stream)."""

    def __init__(self, device=None, serial=False, parse_only=False, small_segments=False, opts=0, ctx=None):
        """serial: the one-lane exact chase (XYWS_OPT_SERIAL_SCAN). small_segments:
        test geometry of the run-parallel decoder (1 KiB runs), so that small
        inputs cross many run boundaries (speculated entries and their repair).
        opts: further XYWS_OPT_* bits. ctx: a Context of its own (default: the
        thread's context for the device)."""
        import torch
        self.ctx = ctx if ctx is not None else context(device)
        self.device = torch.device("cuda", self.ctx.device)
        self.carry_t = torch.zeros(64, dtype=torch.uint8, device=self.device)
        self.opts = ((_lib.OPT_SERIAL_SCAN if serial else 0) | (_lib.OPT_PARSE_ONLY if parse_only else 0) |
                     (_lib.OPT_SMALL_SEG if small_segments else 0) | opts)

    def reset(self):
        self.carry_t.zero_()

    def carry(self):
        return Carry.from_buffer_copy(self.carry_t.cpu().numpy().tobytes())

    def decode(self, buf, cap=0, count=True, carry=True):
        """Decode one batch in place. cap: frame descriptors to return; count:
        return the frame count; carry=False decodes the batch as a fresh stream
        and keeps no state (no carry read or written)."""
        import torch
        t = _dev_u8(buf)
        frames_t = torch.empty(max(cap, 1) * 32, dtype=torch.uint8, device=self.device) if cap else None
        n_t = torch.zeros(1, dtype=torch.int64, device=self.device) if count else None
        cp = C.c_void_p(self.carry_t.data_ptr()) if carry else None
        check(self.ctx.L.xyws_decode_stream(
            self.ctx.h, C.c_void_p(t.data_ptr()), t.numel(), cp, cp,
            C.c_void_p(frames_t.data_ptr()) if frames_t is not None else None, cap,
            C.c_void_p(n_t.data_ptr()) if n_t is not None else None, self.opts, _stream(t)),
            "xyws_decode_stream")
        return DecodeResult(frames_t, n_t, cap)

    def decode_iov(self, bufs, cap=0, count=True, carry=True):
        """Decode a buffer sequence (device uint8 tensors, one recv's pieces)
        as ONE stream, every piece in place (xyws_decode_stream_iov: a single
        piece or few large ones where they lie, else gathered, decoded and
        scattered back in three launches). Descriptor offsets count bytes
        across the pieces in order."""
        import torch
        ts = [_dev_u8(b) for b in bufs]
        arr = (C.c_uint64 * (2 * max(len(ts), 1)))()
        for k, t in enumerate(ts):
            arr[2 * k], arr[2 * k + 1] = t.data_ptr(), t.numel()
        frames_t = torch.empty(max(cap, 1) * 32, dtype=torch.uint8, device=self.device) if cap else None
        n_t = torch.zeros(1, dtype=torch.int64, device=self.device) if count else None
        cp = C.c_void_p(self.carry_t.data_ptr()) if carry else None
        check(self.ctx.L.xyws_decode_stream_iov(
            self.ctx.h, C.cast(arr, C.c_void_p), len(ts), cp, cp,
            C.c_void_p(frames_t.data_ptr()) if frames_t is not None else None, cap,
            C.c_void_p(n_t.data_ptr()) if n_t is not None else None, self.opts,
            _stream(ts[0]) if ts else C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
            "xyws_decode_stream_iov")
        return DecodeResult(frames_t, n_t, cap)


def _set_out(row, t):
    """A row's out, out_cap pair: the tensor t."""
    row.out, row.out_cap = t.data_ptr(), t.numel()


class _Done:
    """The event behind the last call that was marked: wait() returns when that call has run."""

    def __init__(self):
        self.event = None

    def wait(self):
        if self.event is not None:
            self.event.synchronize()

    def mark(self, stream):
        import torch
        self.event = torch.cuda.Event()
        self.event.record(stream)


class _Slot(_Done):
    """One slot of a connection_group's ring: a pinned and a device tensor
    for each table a sweep uploads (xyws_conn, xyws_reply_conn,
    xyws_reasm_conn), and the event of the last call that read them. A pinned
    table is rewritten only after its copy and its call have run: wait()."""

    def __init__(self, n, device):
        super().__init__()
        structs = (_lib.Conn, _lib.ReplyConn, _lib.ReasmConn)
        self.host = {s: _lib.alloc_rows(s, n, "cpu").pin_memory() for s in structs}
        self.dev = {s: _lib.alloc_rows(s, n, device, zero=False) for s in structs}

    def upload(self, struct, m, fill):
        """The slot's table of m `struct` rows on the device, each row set by fill(row, k)."""
        tab = _lib.Table(struct, m, self.host[struct])
        for k in range(m):
            fill(tab[k], k)
        return tab.upload(self.dev[struct])


class GroupResult:
    """Counts and frames of one connection_group.decode call, item k being the
    k-th (conn_id, buffer) pair of that call (host copies on demand). They
    live in the group's tensors: valid until the group's next decode."""

    def __init__(self, group, ids, conns_t, slot=None, resident=False):
        """conns_t: the device xyws_conn table the call ran over; slot: the
        ring slot that holds it, which reply() and reassemble() put their own
        tables into; resident: the table is the one inbox() keeps."""
        self.group, self.ids = group, ids
        self.conns_t, self.slot, self.resident = conns_t, slot, resident
        self._counts = None
        self._replied = self._reassembled = False  # (a second reply() or reassemble() rewrites the slot's table)

    def nframes(self, k):
        if self._counts is None:
            self._counts = self.group.counts_t[:max(len(self.ids), 1)].cpu().tolist()
        if not 0 <= k < len(self.ids):
            raise IndexError(k)
        return self._counts[k]

    def frames(self, k):
        g = self.group
        return _lib.read_rows(Frame, g.frames_t, min(self.nframes(k), g.cap), g.cap * self.ids[k])


class GroupReply:
    """Results and verdicts of one connection_group.reply call, item k as in
    the decode result it answered (host copies on demand; valid until the
    group's next reply). outs: the send tensors it wrote, which outbox() packs."""

    def __init__(self, group, decoded, outs):
        self.group, self.decoded, self.outs = group, decoded, outs
        self._rows = _Rows(_lib.ReplyResult, group.results_t, len(decoded.ids))

    def result(self, k):
        """xyws_reply_result of item k."""
        return self._rows[k]

    def verdicts(self, k):
        """The verdicts of item k's frames (empty when its reply overflowed or the connection was closed)."""
        g, res = self.group, self.result(k)
        if res.status & _lib.RPL_OVERFLOW or (res.status & _lib.RPL_CLOSED and res.first_close == _lib.NPOS):
            return []
        n = min(self.decoded.nframes(k), g.cap)
        return _lib.read_rows(_lib.Verdict, g.verdicts_t, n, g.cap * self.decoded.ids[k])


class GroupAccept:
    """Verdicts and responses of one connection_group.accept call, item k
    being the k-th request of that call (host copies on demand). The call
    keeps no state in the group: the rows and the table belong to this
    object."""

    def __init__(self, group, ids, outs, table_t, results_t):
        self.group, self.ids, self.outs = group, ids, outs
        self._table_t, self.results_t = table_t, results_t  # (the table stays alive until the call has run)
        self._rows = _Rows(_lib.AcceptResult, results_t, len(outs))

    def result(self, k):
        """xyws_accept_result of item k."""
        return self._rows[k]

    def response(self, k):
        """The response bytes written to item k's send buffer (empty while its request is incomplete)."""
        res = self.result(k)
        n = min(res.resp_len, self.outs[k].numel())
        return self.outs[k][:n].cpu().numpy().tobytes() if n else b""


class RouteTable:
    """A route table on the device (connection_group.routes): the blob
    xyws_route_build makes of the exact and the prefix routes, kept resident
    and passed to every route() call; update() replaces it."""

    def __init__(self, group, exact=None, prefix=None, slots=0):
        self.group, self.blob_t, self.nbytes, self.host = group, None, 0, b""
        self.update(exact, prefix, slots)

    def update(self, exact=None, prefix=None, slots=0):
        """Replace the routes (the calls already queued keep reading the old blob's storage in stream order)."""
        import numpy as np
        import torch
        self.host = _lib.route_table(exact, prefix, slots)
        fresh = torch.from_numpy(np.frombuffer(self.host, np.uint8).copy())
        if self.blob_t is None or self.blob_t.numel() < len(self.host):
            self.blob_t = fresh.to(self.group.device)
        else:
            self.blob_t[:len(self.host)].copy_(fresh)
        self.nbytes = len(self.host)
        return self


class GroupRoute:
    """Results of one connection_group.route call, item k being item k of
    the accept() call it took (host copies on demand). It owns the
    xyws_roster_conn rows the call wrote the rooms into, which
    roster(route=...) completes and hands to xyws_roster_streams."""

    def __init__(self, group, accept, table, rconn_of, tensors):
        self.group, self.accept, self.table, self.rconn_of, self._tensors = group, accept, table, rconn_of, tensors
        self.rconns_t = tensors["rconns"]
        self._rows = _Rows(_lib.RouteResult, tensors["results"], len(accept.ids))

    def result(self, k):
        """xyws_route_result of item k."""
        return self._rows[k]

    def _complete(self, fresh, keep_rows):
        """The host-built roster rows `fresh` over this call's rows, the room
        words of keep_rows excepted: those are the ones the device wrote."""
        import torch
        col = _lib.RosterConn.room.offset // 4
        dst = self.rconns_t.view(torch.int32).view(-1, C.sizeof(_lib.RosterConn) // 4)
        src = fresh.view(torch.int32).view(-1, C.sizeof(_lib.RosterConn) // 4)
        idx = torch.tensor(sorted(keep_rows), dtype=torch.long).to(self.group.device)
        kept = dst[idx, col].clone()
        dst.copy_(src[:dst.shape[0]])
        dst[idx, col] = kept
        return self.rconns_t


class GroupMessages:
    """Results and message records of one connection_group.reassemble call,
    item k as in the decode result it took (host copies on demand; valid until
    the group's next reassemble). outs: the message tensors it wrote (hold()
    looks in front of them); out_caps: their sizes (broadcast() sizes the
    wires by them)."""

    def __init__(self, group, decoded, msg_cap, outs):
        self.group, self.decoded, self.msg_cap, self.outs = group, decoded, msg_cap, outs
        self.out_caps = [t.numel() for t in outs]
        self._rows = _Rows(_lib.ReasmResult, group.mresults_t, len(decoded.ids))

    def tables(self):
        """The xyws_reasm_conn table and the result rows that broadcast() and backlog() read (device tensors)."""
        return self.decoded.slot.dev[_lib.ReasmConn], self.group.mresults_t

    def result(self, k):
        """xyws_reasm_result of item k."""
        return self._rows[k]

    def messages(self, k):
        """The stored records of item k (xyws_message; out_off counts from its out buffer's start)."""
        g = self.group
        n = min(self.result(k).nmsgs, self.msg_cap)
        return _lib.read_rows(_lib.Message, g.msgs_t, n, (g.cap + 1) * self.decoded.ids[k])


class GroupHold:
    """The view and results of one connection_group.hold call, item k as in
    the decode result of its sweep (host copies on demand). broadcast() takes
    it in place of the reassemble() result: in the sweep that completes a
    message a recv boundary cut, the view names the whole message. It owns the
    call's tables, view rows and result rows."""

    def __init__(self, group, messages, tensors, hold_cap):
        self.group, self.decoded, self.messages_in = group, messages.decoded, messages
        self._tensors, self.hold_cap = tensors, hold_cap
        self.msg_cap = messages.msg_cap
        self.out_caps = [c + hold_cap for c in messages.out_caps]  # (broadcast() sizes the wires by them)
        self._rows = _Rows(_lib.HoldResult, tensors["results"], len(self.decoded.ids))
        self._vrows = _Rows(_lib.ReasmResult, tensors["view_results"], len(self.decoded.ids))

    def tables(self):
        """The view and its result rows, which broadcast() and backlog() read instead of the reassembly's."""
        return self._tensors["view"], self._tensors["view_results"]

    def result(self, k):
        """xyws_hold_result of item k."""
        return self._rows[k]

    def view_result(self, k):
        """Item k's row of the view (xyws_reasm_result)."""
        return self._vrows[k]

    def messages(self, k):
        """The view's stored records of item k (out_off counts from the hold's
        start, hold_cap bytes in front of its out buffer)."""
        n = min(self.view_result(k).nmsgs, self.msg_cap)
        return _lib.read_rows(_lib.Message, self._tensors["vmsgs"], n, (self.group.cap + 1) * k)


class GroupBroadcast:
    """Results, room results and wires of one connection_group.broadcast call,
    item k as in the decode result of its sweep, room r as in the `rooms`
    argument (host copies on demand). It owns the call's tables, wires and
    result rows. The sweep's later calls read its fields: messages (the
    reassemble() or hold() result it delivered), outs and heads (per item),
    replied (whether the sweep's reply rows are named), room_set (None over
    lists) and the table tensors."""

    def __init__(self, group, messages, outs, heads, replied, wires, tensors, room_set=None):
        self.group, self.decoded, self.messages = group, messages.decoded, messages
        self.outs, self.heads, self.replied, self.room_set = outs, heads, replied, room_set
        self._tensors, self._wires = tensors, wires
        self.members_t, self.rooms_t, self.bconns_t = tensors["members"], tensors["rooms"], tensors["bconns"]
        self.results_t, self.room_results_t = tensors["results"], tensors["room_results"]
        self._rows = _Rows(_lib.BcastResult, self.results_t, len(self.decoded.ids))
        self._rrows = _Rows(_lib.RoomResult, self.room_results_t, len(wires))

    def result(self, k):
        """xyws_bcast_result of item k."""
        return self._rows[k]

    def room_result(self, r):
        """xyws_room_result of room r."""
        return self._rrows[r]

    def wire(self, r):
        """Room r's outbound bytes of this sweep (a device tensor: the first
        min(wire_len, wire_cap) bytes)."""
        res = self.room_result(r)
        return self._wires[r][:min(res.wire_len, self._wires[r].numel())]


class GroupBacklog:
    """Results of one connection_group.backlog call: item k as in the decode
    result of its sweep, room r as in the broadcast's `rooms` argument (host
    copies on demand). The logs and carries belong to the group. bcast: the
    sweep's GroupBroadcast; roster: its GroupRoster, or None."""

    def __init__(self, group, bcast, roster, tensors, nr):
        self.group, self.decoded, self.bcast, self.roster = group, bcast.decoded, bcast, roster
        self._tensors, self.nr = tensors, nr
        self.results_t = tensors["results"]
        self._rows = _Rows(_lib.BacklogResult, self.results_t, len(self.decoded.ids))
        self._rrows = _Rows(_lib.BacklogRoomResult, tensors["room_results"], nr)

    def result(self, k):
        """xyws_backlog_result of item k."""
        return self._rows[k]

    def room_result(self, r):
        """xyws_backlog_room_result of room r."""
        return self._rrows[r]


class RoomSet:
    """The rooms of a connection_group kept on the device
    (connection_group.rooms): the xyws_room table, every room's member array
    of member_cap entries, its wire and its notice buffer, and the group's
    xyws_bcast_conn table, whose room column says where each connection is.
    roster() rewrites the lists, the counts and that column on the device;
    broadcast() reads them. A second table of the same shape (the `seen`
    rows) receives each sweep's lists as its broadcast read them: backlog()
    behind a roster() folds from those, so a member that talks and closes in
    one sweep, or a joiner that spoke, does not cost the room its recent
    messages. Connection k is item k of every sweep."""

    def __init__(self, group, n_rooms, member_cap, wire_cap, notes_cap):
        import torch
        self.group, self.nr, self.member_cap = group, int(n_rooms), int(member_cap)
        if self.nr < 0 or self.member_cap < 0 or wire_cap < 1 or notes_cap < 1:
            raise ValueError("n_rooms and member_cap must not be negative, the buffers not empty")
        dev, n = group.device, group.n
        with torch.cuda.device(dev):
            self.members_t = torch.zeros(max(self.nr * self.member_cap, 1), dtype=torch.int32, device=dev)
            self.wires = [torch.empty(int(wire_cap), dtype=torch.uint8, device=dev) for _ in range(self.nr)]
            self.notes = [torch.empty(int(notes_cap), dtype=torch.uint8, device=dev) for _ in range(self.nr)]
            # the `seen` rows: each sweep's lists as its broadcast read them, for that sweep's backlog fold
            self.seen_members_t = torch.zeros(max(self.nr * self.member_cap, 1), dtype=torch.int32, device=dev)
            rtab, stab = _lib.Table(_lib.Room, self.nr), _lib.Table(_lib.Room, self.nr)
            self.seen_rooms_t = _lib.alloc_rows(_lib.Room, self.nr, dev)
            rrtab = _lib.Table(_lib.RosterRoom, self.nr)
            for r in range(self.nr):
                rtab[r].members, rtab[r].n_members = self.members_t.data_ptr() + 4 * self.member_cap * r, 0
                stab[r].members, stab[r].n_members = self.seen_members_t.data_ptr() + 4 * self.member_cap * r, 0
                for row in (rtab[r], stab[r]):
                    row.wire, row.wire_cap = self.wires[r].data_ptr(), self.wires[r].numel()
                rrtab[r].member_cap = self.member_cap
                rrtab[r].notes, rrtab[r].notes_cap = self.notes[r].data_ptr(), self.notes[r].numel()
                rrtab[r].seen = _lib.row_ptr(self.seen_rooms_t, _lib.Room, r)
            self.seen_rooms_t.copy_(stab.upload(dev))
            self.rooms_t, self.rrooms_t = rtab.upload(dev), rrtab.upload(dev)
            btab = _lib.Table(_lib.BcastConn, n)
            for k in range(n):
                btab[k].room = _lib.ROOM_NONE
            self.bconns_t = btab.upload(dev)

    def stage_bconns(self, table):
        """The caller's fields of the bconns rows (head .. reply) from a
        host-built table, on the device; the room column stays the roster's."""
        import torch
        n, words = self.group.n, _lib.BcastConn.room.offset // 8
        with torch.cuda.device(self.group.device):
            fresh = table.upload(self.group.device).view(torch.int64).view(max(n, 1), -1)
            self.bconns_t.view(torch.int64).view(max(n, 1), -1)[:n, :words].copy_(fresh[:n, :words])

    def members(self, r):
        """Host copy of room r's list (synchronizes)."""
        if not 0 <= r < self.nr:
            raise IndexError("no such room")
        count = _lib.read_rows(_lib.Room, self.rooms_t, 1, r)[0].n_members
        lo = self.member_cap * r
        return [int(x) & 0xFFFFFFFF for x in self.members_t[lo:lo + count].cpu().numpy()]

    def state_tensors(self):
        """The tensors roster() rewrites from sweep to sweep."""
        return [self.members_t, self.rooms_t, self.bconns_t]


class GroupRoster:
    """Results of one connection_group.roster call: item k as in the decode
    result of its sweep, room r as in the room set (host copies on demand). It
    owns the call's tables and rows; the lists belong to the room set."""

    def __init__(self, group, bcast, room_set, tensors):
        self.group, self.bcast, self.room_set, self._tensors = group, bcast, room_set, tensors
        self.decoded = bcast.decoded
        self.results_t, self.jconns_t = tensors["results"], tensors["jconns"]  # (outbox() and backlog() name them)
        self._rows = _Rows(_lib.RosterResult, self.results_t, len(self.decoded.ids))
        self._rrows = _Rows(_lib.RosterRoomResult, tensors["room_results"], room_set.nr)

    def result(self, k):
        """xyws_roster_result of item k."""
        return self._rows[k]

    def room_result(self, r):
        """xyws_roster_room_result of room r."""
        return self._rrows[r]

    def notes(self, r):
        """Room r's notice wire of this sweep (a device tensor: the first min(notes_len, notes_cap) bytes)."""
        t = self.room_set.notes[r]
        return t[:min(self.room_result(r).notes_len, t.numel())]

    def members(self, r):
        """Room r's list after the call (host copy)."""
        return self.room_set.members(r)


class GroupOutbox:
    """The pack, send list and summary of one connection_group.outbox call
    (host copies on demand; every accessor waits for the call). Table row i is
    item i of the sweep; the rows behind the sweep's items are the accept()
    items that are no item of the sweep. conn_ids[i] is row i's connection id.
    It owns the call's table, outputs and scratch."""

    def __init__(self, group, conn_ids, outs, tensors, pack_cap, host, last, accept, done):
        self.group, self.conn_ids, self.outs, self._tensors = group, conn_ids, outs, tensors
        self.pack_cap, self.host = pack_cap, host
        self.last, self.accept, self._done = last, accept, done  # (the sweep's results, whose rows the table names)
        self._summary = self._entries = self._pack = None

    def summary(self):
        """xyws_outbox_summary of the call."""
        if self._summary is None:
            self._done.wait()
            self._summary = _lib.read_rows(_lib.OutboxSummary, self._tensors["summary"], 1)[0]
        return self._summary

    def entries(self):
        """The send list: the n_entries xyws_outbox_entry rows, in table order."""
        if self._entries is None:
            self._entries = _lib.read_rows(_lib.OutboxEntry, self._tensors["entries"], self.summary().n_entries)
        return self._entries

    def pack(self):
        """The first packed_len bytes of the pack (host bytes)."""
        if self._pack is None:
            n = self.summary().packed_len
            self._pack = self._tensors["pack"][:n].cpu().numpy().tobytes() if n else b""
        return self._pack

    def bytes(self, k):
        """The bytes entry k sends: its slot of the pack, or for a deferred
        entry the first len bytes of its send tensor."""
        e = self.entries()[k]
        if e.flags & _lib.OB_DEFERRED:
            return self.outs[e.conn][:e.len].cpu().numpy().tobytes()
        return self.pack()[e.off:e.off + e.len]


class GroupInbox:
    """Results of one connection_group.inbox call (host copies on demand; every
    accessor waits for the call). Row i is connection i of the group: the
    tables behind it are the group's resident ones, which decode() and accept()
    take in place of their item lists. The result rows, the xyws_conn rows and
    the receive slab live in the group's tensors: result(), conn() and
    received() are valid until the group's next inbox() call (a row read
    before that stays as it was read); summary() belongs to this object."""

    def __init__(self, group, tensors, m, done):
        self.group, self._tensors, self.m, self._done = group, tensors, m, done
        self.ids = list(range(group.n))
        self._summary = self._rows = None

    def summary(self):
        """xyws_inbox_summary of the call."""
        if self._summary is None:
            self._done.wait()
            self._summary = _lib.read_rows(_lib.InboxSummary, self._tensors["summary"], 1)[0]
        return self._summary

    def result(self, k):
        """xyws_inbox_result of connection k."""
        if self._rows is None:
            self._done.wait()
            self._rows = _lib.read_rows(_lib.InboxResult, self._tensors["results"], self.group.n)
        return self._rows[k]

    def conn(self, k):
        """Host copy of connection k's resident xyws_conn row (synchronizes)."""
        return _lib.read_rows(_lib.Conn, self.group._ib["conns"], 1, k)[0]

    def received(self, k):
        """The bytes connection k's xyws_conn row names after the call: what decode() reads (synchronizes)."""
        g, row = self.group, self.conn(k)
        off = row.buf - g._ib["slab"].data_ptr()
        return g._ib["slab"][off:off + row.len].cpu().numpy().tobytes() if row.len else b""


class connection_group:
    """The decoder states of n connections and one xyws_decode_streams call
    for whatever a sweep of the completion queue brought: decode() takes the
    (conn_id, device buffer) pairs of the connections that received bytes
    and decodes them all in one launch, each from its own device-resident
    carry, as frame_decoder.decode would one by one. Owns the carries (n x 64
    bytes, zeroed), a descriptor table of cap rows per connection and a count
    vector. reply() then answers what decode() found, again in one launch
    (xyws_reply_streams): a whole echo sweep is two launches. reassemble()
    gathers and validates the messages of what decode() found, in one launch
    too (xyws_reassemble_streams), before or after reply(). broadcast() then
    delivers those messages to their rooms (xyws_broadcast_streams): each
    room's wire behind every member's reply. hold(), between the two, keeps
    the parts of a message a recv boundary cut on the device
    (xyws_hold_streams) and hands broadcast() the whole message in the sweep
    that completes it. backlog(), after broadcast(), keeps each room's recent
    messages on the device (xyws_backlog_streams) and sends them to the
    connections that join. rooms() makes a room set that lives on the device;
    with it broadcast() reads the lists where roster(), between broadcast()
    and backlog(), keeps them (xyws_roster_streams): joins and leaves taken
    from the sweep's own rows, each said to the room as the reference's
    welcome and farewell lines. outbox() ends the sweep (xyws_outbox_streams):
    every connection's send bytes in one pack, with the list of who sends and
    who is closed, in device or pinned host memory. inbox()
    (xyws_inbox_streams) is a receive path of its own so far: a dense pack of
    the received bytes and one entry per completed recv scattered into a
    receive slab the group owns, with resident n-row tables that accept() and
    decode() then run over. What decode() returns for a GroupInbox gives counts
    and frames; reply(), reassemble(), hold() and broadcast() take only the
    result of a decode() over (conn_id, buffer) pairs, so in Python a sweep that
    starts with inbox() ends at decode().

    The tables decode(), reply() and reassemble() upload go through one ring
    of RING slots (_Slot): decode() takes the next slot, the sweep's later
    calls use the slot of the decode() result they are given and move its
    event behind themselves. Every xyws_*_streams call is made by _call()."""
    RING = 4  # tables in flight: a pinned table is rewritten only after its copy and its call have run

    def __init__(self, n, cap=0, device=None, ctx=None, parse_only=False):
        import torch
        self.ctx = ctx if ctx is not None else context(device)
        self.device = dev = torch.device("cuda", self.ctx.device)
        self.n, self.cap = n, cap = int(n), int(cap)
        self.opts = _lib.OPT_PARSE_ONLY if parse_only else 0
        self.carry_t = _lib.alloc_rows(Carry, n, dev)
        self.frames_t = _lib.alloc_rows(Frame, n * cap, dev, zero=False)
        self.counts_t = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        self._ring = [_Slot(n, dev) for _ in range(self.RING)]
        self._turn = 0
        # reply(): the reply carries, a verdict row of cap per connection, a result row per item
        self.rcarry_t = _lib.alloc_rows(_lib.ReplyCarry, n, dev)
        self.verdicts_t = _lib.alloc_rows(_lib.Verdict, n * cap, dev, zero=False)
        self.results_t = _lib.alloc_rows(_lib.ReplyResult, n, dev)
        # reassemble(): the message carries, a record row of cap + 1 per connection, a result row per item
        self.mcarry_t = _lib.alloc_rows(_lib.MsgCarry, n, dev)
        self.msgs_t = _lib.alloc_rows(_lib.Message, n, dev, zero=False, per=cap + 1)
        self.mresults_t = _lib.alloc_rows(_lib.ReasmResult, n, dev)
        # hold(): the hold carries (its tables and rows belong to the GroupHold it returns)
        self.hcarry_t = _lib.alloc_rows(_lib.HoldCarry, n, dev)
        # backlog(): per room a log and a carry, made when the room is first seen and kept across sweeps
        self._blogs, self._bcarries = [], []
        # inbox(): the receive slab, the inbox carries and the resident tables, made by the first inbox() call
        self._ib = None

    def _call(self, name, *args, slot=None, done=None):
        """One call of the library on the group's device and its current
        stream: getattr(L, name)(ctx, *args, stream), a tensor argument passed
        as its address. The function is looked up when the call is made.
        slot, done: the ring slot and the result's _Done whose events move
        behind the call."""
        import torch
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
            check(getattr(self.ctx.L, name)(self.ctx.h, *args, stream.cuda_stream), name)
            for d in (slot, done):
                if d is not None:
                    d.mark(stream)

    def _carries(self):
        """The per-connection state a slot loses when it changes hands, as (tensor, row structure) pairs."""
        pairs = [(self.carry_t, Carry), (self.rcarry_t, _lib.ReplyCarry), (self.mcarry_t, _lib.MsgCarry),
                 (self.hcarry_t, _lib.HoldCarry)]
        if self._ib is not None:
            pairs += [(self._ib["carries"], _lib.InboxCarry), (self._ib["aresults"], _lib.AcceptResult)]
        return pairs

    def reset(self, ids=None):
        """Fresh streams: every connection, or those in `ids`. A slot that
        changes hands also loses the handshake verdict of the connection
        before it: its inbox carry and its resident xyws_accept_result row are
        both zeroed, or the next inbox() call would open or refuse the new
        connection by the old one's row."""
        ids = None if ids is None else list(ids)
        for t, struct in self._carries():
            if ids is None:
                t.zero_()
            else:
                size = C.sizeof(struct)
                for i in ids:
                    t[size * i:size * (i + 1)].zero_()

    def _carry_of(self, t, struct, conn_id):
        """Host copy of connection conn_id's row of a carry tensor (synchronizes)."""
        if not 0 <= conn_id < self.n:
            raise XywsError(-1, "no such connection")
        return _lib.read_rows(struct, t, 1, conn_id)[0]

    def carry(self, conn_id):
        """Host copy of a connection's carry (synchronizes)."""
        return self._carry_of(self.carry_t, Carry, conn_id)

    def _conn_row(self, row, buf, length, i):
        """Connection i's xyws_conn row over `length` bytes at the device address buf."""
        row.buf, row.len, row.carry = buf, length, _lib.row_ptr(self.carry_t, Carry, i)
        row.frames, row.cap = (_lib.row_ptr(self.frames_t, Frame, self.cap * i), self.cap) if self.cap else (0, 0)

    def decode(self, items):
        """items: (conn_id, device uint8 tensor) pairs, each id at most once.
        Every buffer is decoded in place; returns a GroupResult. A GroupInbox
        in place of the pairs decodes every connection of the group over the
        resident xyws_conn table that inbox() keeps: item k is connection k.
        That result gives nframes() and frames() only: reply(), reassemble(),
        hold() and broadcast() refuse it (they need the table of a decode()
        over pairs)."""
        if isinstance(items, GroupInbox):
            if items.group is not self:
                raise XywsError(-1, "decode() takes a GroupInbox of this group")
            conns_t = self._ib["conns"]
            self._call("xyws_decode_streams", conns_t, self.n, self.counts_t, self.opts)
            return GroupResult(self, list(range(self.n)), conns_t, resident=True)
        items = [(int(i), _dev_u8(t)) for i, t in items]
        ids = [i for i, _ in items]
        if len(set(ids)) != len(ids) or any(not 0 <= i < self.n for i in ids):
            raise XywsError(-1, "connection ids must be distinct and below n")
        if any(t.device != self.device for _, t in items):
            raise XywsError(-1, "a buffer on another device than the group's")
        slot = self._ring[self._turn]
        self._turn = (self._turn + 1) % self.RING
        slot.wait()

        def fill(row, k):
            i, t = items[k]
            self._conn_row(row, t.data_ptr(), t.numel(), i)
        conns_t = slot.upload(_lib.Conn, len(items), fill)
        self._call("xyws_decode_streams", conns_t, len(items), self.counts_t, self.opts, slot=slot)
        return GroupResult(self, ids, conns_t, slot)

    def accept(self, items, out_items, policy=0, max_request=1024):
        """Answer the opening handshakes of the connections still in HTTP
        state (xyws_accept_streams, one launch), before decode() sees them:
        items[k] is the device uint8 tensor with every byte connection k has
        sent so far (or a (conn_id, tensor) pair; the ids are only kept for
        the caller), out_items[k] the device uint8 tensor that receives its
        response (129 bytes always suffice). A whole request is checked by
        RFC 6455 4.2.1 (policy 0) or as the reference's handler does
        (ACC_REFERENCE) and answered; an incomplete one is reported as such:
        call again with more bytes. The call keeps no state: on ACCEPTED the
        bytes behind result(k).consumed are the connection's first decode()
        input. A GroupInbox in place of the items runs over the resident
        xyws_accept_conn table that inbox() keeps (item k is connection k, the
        responses go to the group's own response slab, out_items is None), and
        the next inbox() call reads the rows this call leaves. The rows and
        responses of that GroupAccept live in the group's tensors: they are
        valid until the group's next accept() over a GroupInbox, or until
        reset() clears a slot's row. Returns a GroupAccept."""
        if isinstance(items, GroupInbox):
            if items.group is not self or out_items is not None:
                raise XywsError(-1, "accept() takes a GroupInbox of this group and no send buffers with it")
            ib = self._ib
            ids = list(range(self.n))
            outs = [ib["resp"][ib["resp_cap"] * i:ib["resp_cap"] * (i + 1)] for i in ids]
            table_t, results_t = ib["aconns"], ib["aresults"]
        else:
            pairs = [it if isinstance(it, tuple) else (k, it) for k, it in enumerate(items)]
            ids = [int(i) for i, _ in pairs]
            bufs = [_dev_u8(t) for _, t in pairs]
            outs = [_dev_u8(t) for t in out_items]
            if len(outs) != len(bufs) or any(t.device != self.device for t in bufs + outs):
                raise XywsError(-1, "one request and one send buffer on the group's device per item")
            tab = _lib.Table(_lib.AcceptConn, len(bufs))
            for row, b, o in zip(tab.rows, bufs, outs):
                row.buf, row.len = b.data_ptr(), b.numel()
                _set_out(row, o)
            table_t = tab.upload(self.device)
            results_t = _lib.alloc_rows(_lib.AcceptResult, len(bufs), self.device)
        self._call("xyws_accept_streams", table_t, len(ids), int(max_request), int(policy), results_t)
        return GroupAccept(self, ids, outs, table_t, results_t)

    def routes(self, exact=None, prefix=None, slots=0):
        """A route table on the device: exact = {key bytes: room} matches a
        request target's key (the target up to its first `?` or `#`, one
        trailing `/` dropped) byte for byte, prefix = {key bytes: room} also
        every key below it (`/rooms` matches `/rooms/a`, `/` everything that
        begins with `/`); the longest key wins. Returns a RouteTable."""
        return RouteTable(self, exact, prefix, slots)

    def route(self, accept, table, rconn_of=None, default_room=_lib.ROOM_NONE, miss_404=False):
        """Send every connection that accept() accepted to the room its
        request target names (xyws_route_streams, one launch), between
        accept() and roster(): rconn_of[k] is the roster row (the connection
        id of the sweep) of accept item k, None for none; by default the ids
        given to accept(). A target no route matches goes to default_room, or
        with miss_404 gets `404 Not Found` over its 101 and counts as a
        rejected handshake from then on. Returns a GroupRoute, which
        roster(route=...) takes."""
        if not isinstance(accept, GroupAccept) or accept.group is not self or not isinstance(table, RouteTable) or \
                table.group is not self:
            raise XywsError(-1, "route() takes this group's accept() result and one of its route tables")
        m = len(accept.ids)
        if rconn_of is None:
            rconn_of = dict(enumerate(accept.ids))
        elif not isinstance(rconn_of, dict):
            rconn_of = dict(enumerate(rconn_of))
        rconn_of = {int(k): int(r) for k, r in rconn_of.items() if r is not None}
        rows = list(rconn_of.values())
        if any(not 0 <= k < m for k in rconn_of) or any(not 0 <= r < self.n for r in rows) or len(set(rows)) != len(rows):
            raise XywsError(-1, "rconn_of names accept items and distinct connections of the group")
        tab = _lib.Table(_lib.RouteConn, m)
        for k in range(m):
            tab[k].rconn = rconn_of.get(k, _lib.ROUTE_NO_ROW)
        rtab = _lib.Table(_lib.RosterConn, self.n)
        for i in range(self.n):
            rtab[i].room = _lib.ROOM_NONE
        tensors = dict(rtconns=tab.upload(self.device), rconns=rtab.upload(self.device),
                       results=_lib.alloc_rows(_lib.RouteResult, m, self.device))
        self._call("xyws_route_streams", accept._table_t, accept.results_t, tensors["rtconns"], m, table.blob_t,
                   table.nbytes, tensors["rconns"], self.n, int(default_room), _lib.RT_MISS_404 if miss_404 else 0,
                   tensors["results"])
        return GroupRoute(self, accept, table, rconn_of, tensors)

    def reply_carry(self, conn_id):
        """Host copy of a connection's reply carry (synchronizes)."""
        return self._carry_of(self.rcarry_t, _lib.ReplyCarry, conn_id)

    def reply(self, result, out_items, max_payload, policy=0, flags=0x11, enc_opts=0, action_mask=1):
        """Answer the frames of the decode() call that returned `result`
        (xyws_reply_streams, one launch): out_items[k] is the device uint8
        tensor that receives item k's reply (len + 13 bytes always suffice).
        Every answered frame is echoed with `flags` (default FIN | TEXT, the
        reference's echo_once), or with XYWS_ENC_FRAME_OPCODE under its own
        opcode; action_mask selects the verdict actions that are answered; a
        frame the policy closes on ends the reply with the close frame. The
        group owns the reply carries; the verdict rows (cap per connection)
        and the result rows live in its tensors until the next reply().
        Call it before the group's next decode(): the counts are that call's."""
        if result.group is not self or result.resident or not self.cap:
            raise XywsError(-1, "reply() takes the result of this group's decode(), and a group with cap > 0")
        outs = [_dev_u8(t) for t in out_items]
        if len(outs) != len(result.ids) or any(t.device != self.device for t in outs):
            raise XywsError(-1, "one send buffer on the group's device per decoded item")
        slot = result.slot
        if result._replied:
            slot.wait()  # (the slot's reply table is rewritten)
        result._replied = True

        def fill(row, k):
            _set_out(row, outs[k])
            row.rc = _lib.row_ptr(self.rcarry_t, _lib.ReplyCarry, result.ids[k])
            row.verdicts = _lib.row_ptr(self.verdicts_t, _lib.Verdict, self.cap * result.ids[k])
        rconns_t = slot.upload(_lib.ReplyConn, len(outs), fill)
        self._call("xyws_reply_streams", result.conns_t, self.counts_t, rconns_t, len(outs), int(max_payload), policy,
                   flags, enc_opts, action_mask, self.results_t, slot=slot)
        return GroupReply(self, result, outs)

    def reassemble(self, result, out_items, opts=_lib.REASM_UTF8, msg_cap=None):
        """Gather and validate the messages of the decode() call that returned
        `result` (xyws_reassemble_streams, one launch): out_items[k] is the device
        uint8 tensor that receives item k's message bytes (as many bytes as its
        recv buffer held always suffice). Each item is processed as
        message_assembler.feed would process it from the connection's own message
        carry. The group owns the carries; the record rows (cap + 1 per
        connection, msg_cap of them used: default all) and the result rows live in
        its tensors until the next reassemble(). Works before or after reply() on
        the same result; call it before the group's next decode()."""
        if result.group is not self or result.resident or not self.cap:
            raise XywsError(-1, "reassemble() takes the result of this group's decode(), and a group with cap > 0")
        outs = [_dev_u8(t) for t in out_items]
        if len(outs) != len(result.ids) or any(t.device != self.device for t in outs):
            raise XywsError(-1, "one message buffer on the group's device per decoded item")
        mcap = self.cap + 1 if msg_cap is None else int(msg_cap)
        if not 0 <= mcap <= self.cap + 1:
            raise XywsError(-1, "msg_cap above the group's record row (cap + 1)")
        slot = result.slot
        if result._reassembled:
            slot.wait()  # (the slot's table is rewritten)
        result._reassembled = True

        def fill(row, k):
            _set_out(row, outs[k])
            row.mc = _lib.row_ptr(self.mcarry_t, _lib.MsgCarry, result.ids[k])
            row.msgs, row.msg_cap = _lib.row_ptr(self.msgs_t, _lib.Message, (self.cap + 1) * result.ids[k]), mcap
        mconns_t = slot.upload(_lib.ReasmConn, len(outs), fill)
        self._call("xyws_reassemble_streams", result.conns_t, self.counts_t, mconns_t, len(outs), opts,
                   self.mresults_t, slot=slot)
        return GroupMessages(self, result, mcap, outs)

    def hold_carry(self, conn_id):
        """Host copy of a connection's hold carry (synchronizes)."""
        return self._carry_of(self.hcarry_t, _lib.HoldCarry, conn_id)

    def hold(self, messages, hold_cap):
        """Keep the messages that span sweeps (xyws_hold_streams, one launch),
        between reassemble() and broadcast() of the same sweep: `messages` is
        the reassemble() result, and the hold of item k is the hold_cap bytes
        in front of the out tensor reassemble() wrote for it, so every out
        tensor must be a slice that starts at least hold_cap bytes into its
        storage, the same bytes for the connection in every sweep (ValueError
        otherwise). hold_cap >= 2 * (largest message accepted) + 30 always
        suffices. The group owns the hold carries. Returns a GroupHold, which
        broadcast() takes in place of `messages`. Call it before the group's
        next decode(), reply() or reassemble()."""
        dec = messages.decoded
        if messages.group is not self or dec.resident or not isinstance(messages, GroupMessages):
            raise XywsError(-1, "hold() takes the result of this group's reassemble()")
        hold_cap = int(hold_cap)
        if hold_cap < 0:
            raise ValueError("hold_cap must not be negative")
        for k, t in enumerate(messages.outs):
            if t.storage_offset() * t.element_size() < hold_cap:
                raise ValueError(f"item {k}: the out tensor needs hold_cap = {hold_cap} bytes of its storage in front "
                                 f"of it, has {t.storage_offset() * t.element_size()}")
        m, dev = len(dec.ids), self.device
        htab = _lib.Table(_lib.HoldConn, m)
        tensors = dict(vmsgs=_lib.alloc_rows(_lib.Message, m, dev, zero=False, per=self.cap + 1),
                       view=_lib.alloc_rows(_lib.ReasmConn, m, dev),
                       view_results=_lib.alloc_rows(_lib.ReasmResult, m, dev),
                       results=_lib.alloc_rows(_lib.HoldResult, m, dev), outs=messages.outs)
        for k, (row, i) in enumerate(zip(htab.rows, dec.ids)):
            row.hold_cap, row.hc = hold_cap, _lib.row_ptr(self.hcarry_t, _lib.HoldCarry, i)
            row.vmsgs = _lib.row_ptr(tensors["vmsgs"], _lib.Message, (self.cap + 1) * k)
            row.vmsg_cap = messages.msg_cap
        tensors["hold"] = htab.upload(dev)
        self._call("xyws_hold_streams", *messages.tables(), tensors["hold"], m, tensors["view"],
                   tensors["view_results"], tensors["results"], slot=dec.slot)
        return GroupHold(self, messages, tensors, hold_cap)

    def broadcast(self, messages, rooms, out_items, heads=None, reply=None, flags=0x11, enc_opts=0, wire_caps=None):
        """Deliver the whole messages of the reassemble() call that returned
        `messages` (or of the hold() call that followed it: then also the
        messages that call completed) to their rooms (xyws_broadcast_streams, two launches):
        rooms[r] lists the connection ids of room r in delivery order; every
        one must be an item of this sweep (a member that received nothing is
        decoded with an empty buffer) and belongs to one room. Each room's
        messages are framed once with `flags` (default FIN | TEXT, the chat
        writer's; with XYWS_ENC_FRAME_OPCODE each message's own opcode),
        heads[k] (a device uint8 tensor or None) before every message of item
        k, and the room's wire is appended to out_items[k] of every member:
        behind its reply when `reply` is the GroupReply of the same sweep
        (out_items are then the tensors reply() wrote), from the start
        otherwise. wire_caps[r]: room r's wire capacity (default: the bound
        that always suffices). rooms may be the RoomSet of rooms() instead:
        the lists are then the ones roster() keeps on the device, every
        connection of the group is an item of the sweep (item k is connection
        k: XywsError otherwise), and the wires are the room set's. Returns a
        GroupBroadcast. Call it before the group's next decode(), reply() or
        reassemble()."""
        dec = messages.decoded
        if messages.group is not self or dec.resident or not isinstance(messages, (GroupMessages, GroupHold)):
            raise XywsError(-1, "broadcast() takes the result of this group's reassemble() or hold()")
        if reply is not None and (reply.group is not self or reply.decoded is not dec):
            raise XywsError(-1, "reply must be the reply() result of the same sweep")
        outs = [_dev_u8(t) for t in out_items]
        m = len(dec.ids)
        if len(outs) != m or any(t.device != self.device for t in outs):
            raise XywsError(-1, "one send buffer on the group's device per decoded item")
        hds = [None] * m if heads is None else [None if h is None else _dev_u8(h) for h in heads]
        if len(hds) != m or any(h is not None and h.device != self.device for h in hds):
            raise XywsError(-1, "one head (or None) on the group's device per decoded item")
        btab = _lib.Table(_lib.BcastConn, m)
        for k, (row, t, h) in enumerate(zip(btab.rows, outs, hds)):
            row.head, row.head_len = (h.data_ptr(), h.numel()) if h is not None and h.numel() else (0, 0)
            _set_out(row, t)
            row.reply = self._reply_row(k) if reply is not None else 0
        if isinstance(rooms, RoomSet):
            # the lists, the counts and every connection's room are the device's: only the caller's fields are staged
            if rooms.group is not self or list(dec.ids) != list(range(self.n)):
                raise XywsError(-1, "a room set needs slot-stable sweeps: item k is connection k, every connection an item")
            rooms.stage_bconns(btab)
            room_set, wires = rooms, rooms.wires
            tensors = dict(members=rooms.members_t, rooms=rooms.rooms_t, bconns=rooms.bconns_t)
        else:
            room_set = None
            wires, tensors = self._room_tables(messages, rooms, hds, wire_caps, btab)
        nr = len(wires)
        tensors.update(room_results=_lib.alloc_rows(_lib.RoomResult, nr, self.device),
                       results=_lib.alloc_rows(_lib.BcastResult, m, self.device))
        self._call("xyws_broadcast_streams", *messages.tables(), tensors["bconns"], m, tensors["rooms"],
                   tensors["room_results"], nr, flags, enc_opts, tensors["results"], slot=dec.slot)
        return GroupBroadcast(self, messages, outs, hds, reply is not None, wires, tensors, room_set)

    def _reply_row(self, k):
        """The address of item k's xyws_reply_result row."""
        return _lib.row_ptr(self.results_t, _lib.ReplyResult, k)

    def _room_tables(self, messages, rooms, hds, wire_caps, btab):
        """broadcast() over lists: every room's wire, and the member array, the
        xyws_room table and the bconns table (btab with every item's room) on
        the device."""
        import numpy as np
        import torch
        ids_of = messages.decoded.ids
        item = {i: k for k, i in enumerate(ids_of)}
        room_of, flat = {}, []
        for r, ids in enumerate(rooms):
            for i in ids:
                if int(i) not in item or int(i) in room_of:
                    raise XywsError(-1, "a room member must be an item of this sweep and in one room only")
                room_of[int(i)] = r
                flat.append(item[int(i)])
        nr = len(rooms)
        if wire_caps is not None and len(wire_caps) != nr:
            raise XywsError(-1, "one wire capacity per room")
        hlen = [0 if h is None else h.numel() for h in hds]
        wires = []
        for r, ids in enumerate(rooms):
            need = sum(messages.out_caps[item[int(i)]] + messages.msg_cap * (10 + hlen[item[int(i)]]) for i in ids)
            wires.append(torch.empty(max(need if wire_caps is None else int(wire_caps[r]), 1), dtype=torch.uint8,
                                     device=self.device))
        for row, i in zip(btab.rows, ids_of):
            row.room = room_of.get(i, _lib.ROOM_NONE)
        members_t = torch.from_numpy(np.asarray(flat + [0], np.uint32).view(np.uint8)).to(self.device)
        rtab = _lib.Table(_lib.Room, nr)
        pos = 0
        for r, (row, ids) in enumerate(zip(rtab.rows, rooms)):
            cap = wires[r].numel() if wire_caps is None else int(wire_caps[r])
            row.members, row.n_members = members_t.data_ptr() + 4 * pos, len(ids)
            row.wire, row.wire_cap = wires[r].data_ptr() if cap else 0, cap
            pos += len(ids)
        return wires, dict(members=members_t, rooms=rtab.upload(self.device), bconns=btab.upload(self.device))

    def rooms(self, n_rooms, member_cap, wire_cap=65536, notes_cap=65536):
        """A room set on the device: n_rooms rooms of at most member_cap
        members, each with a wire of wire_cap and a notice buffer of notes_cap
        bytes, all empty. broadcast(..., rooms=room_set) reads it, roster()
        keeps it. Returns a RoomSet."""
        return RoomSet(self, n_rooms, member_cap, int(wire_cap), int(notes_cap))

    def roster(self, bcast, room_set, names=None, joins=(), leaves=(), accept=None, on_accept=None,
               leave_on_close=True, flags=0x11, text=None, route=None):
        """Who is in the room (xyws_roster_streams, at most three launches),
        after broadcast(..., rooms=room_set) of the same sweep and before
        backlog(): the room set's lists are updated on the device from the
        sweep's own rows, and every event is said to the room as the
        reference's chat_room says it: a welcome or farewell line framed with
        `flags`, appended behind what broadcast() left in every participant's
        send tensor. names[k]: item k's address text (a device uint8 tensor or
        None); joins: (conn_id, room) pairs; leaves: conn ids; accept with
        on_accept = {conn_id: room}: the GroupAccept of this sweep, whose
        accepted connections join that room behind their 101 in the same send
        tensor; with route, the GroupRoute of this sweep, on_accept may be a
        plain collection of conn ids (and accept is the route's): each joins
        the room route() wrote into its row on the device; leave_on_close: a
        member whose reply closed leaves. text: a
        _lib.RosterText in place of the reference's strings. Nothing is read
        back: the next sweep's broadcast() finds the new lists on the device.
        Returns a GroupRoster, which backlog() takes in place of `bcast`."""
        import torch
        if not isinstance(bcast, GroupBroadcast) or bcast.group is not self or bcast.room_set is not room_set:
            raise XywsError(-1, "roster() takes the result of this group's broadcast() over the same room set")
        dec = bcast.decoded
        m, nr = len(dec.ids), room_set.nr
        nms = [None] * m if names is None else [None if t is None else _dev_u8(t) for t in names]
        if len(nms) != m or any(t is not None and (t.device != self.device or t.numel() > _lib.ROSTER_NAME_MAX)
                                for t in nms):
            raise XywsError(-1, "one name (or None) of at most 256 bytes on the group's device per item")
        ask = {}
        for i, r in list(joins.items() if isinstance(joins, dict) else joins):
            ask[int(i)] = [int(r), _lib.RS_JOIN]
        acc_row, routed = {}, set()
        if route is not None:
            if not isinstance(route, GroupRoute) or route.group is not self or accept not in (None, route.accept):
                raise XywsError(-1, "route is this group's route() result over the accept() result of this sweep")
            accept = route.accept
        if on_accept:
            if accept is None or accept.group is not self:
                raise XywsError(-1, "on_accept needs the accept() result of this sweep")
            acc_row = {i: k for k, i in enumerate(accept.ids)}
            for i, r in (on_accept.items() if isinstance(on_accept, dict) else [(i, None) for i in on_accept]):
                if int(i) not in acc_row or int(i) in ask:
                    raise XywsError(-1, "an on_accept connection must be an item of the accept() call and join once")
                if r is None:  # the room is the one route() wrote into this connection's row
                    if route is None or route.rconn_of.get(acc_row[int(i)]) != int(i):
                        raise XywsError(-1, "an on_accept connection without a room needs the route() result that wrote its row")
                    routed.add(int(i))
                ask[int(i)] = [0 if r is None else int(r), _lib.RS_JOIN_ON_ACCEPT]
        if any(not 0 <= i < m or (i not in routed and not 0 <= r < nr) for i, (r, _) in ask.items()) or \
                any(not 0 <= int(i) < m for i in leaves):
            raise XywsError(-1, "joins and leaves name connections of the group and rooms of the room set")
        gone = {int(i) for i in leaves}
        if text is not None and max(text.head_len, text.joined_len, text.left_len) > _lib.ROSTER_TEXT_MAX:
            raise XywsError(-1, "a text length above 32")
        rtab, jtab = _lib.Table(_lib.RosterConn, m), _lib.Table(_lib.BacklogConn, m)
        results_t = _lib.alloc_rows(_lib.RosterResult, m, self.device)
        for k, (row, jrow, t, nm) in enumerate(zip(rtab.rows, jtab.rows, bcast.outs, nms)):
            row.name, row.name_len = (nm.data_ptr(), nm.numel()) if nm is not None and nm.numel() else (0, 0)
            _set_out(row, t)
            room, fl = ask.get(k, (_lib.ROOM_NONE, 0))
            if k in acc_row and fl & _lib.RS_JOIN_ON_ACCEPT:
                # (the 101 is all this sweep wrote for it)
                row.accept = _lib.row_ptr(accept.results_t, _lib.AcceptResult, acc_row[k])
            else:
                row.bcast = _lib.row_ptr(bcast.results_t, _lib.BcastResult, k)
                row.reply = self._reply_row(k) if bcast.replied else 0
            fl |= (_lib.RS_LEAVE if k in gone else 0) | (_lib.RS_LEAVE_ON_CLOSE if leave_on_close else 0)
            row.room, row.flags = room, fl
            self._backlog_row(jrow, t, k, _lib.row_ptr(results_t, _lib.RosterResult, k),
                              bcast.replied and not row.accept)
        rconns_t = rtab.upload(self.device)
        if routed:
            rconns_t = route._complete(rconns_t, routed)
        tensors = dict(rconns=rconns_t, jconns=jtab.upload(self.device), results=results_t,
                       room_results=_lib.alloc_rows(_lib.RosterRoomResult, nr, self.device),
                       want=torch.zeros(max(m, 1), dtype=torch.int32, device=self.device), names=nms, accept=accept,
                       text=text, route=route)
        self._call("xyws_roster_streams", room_set.bconns_t, rconns_t, m, room_set.rooms_t, room_set.rrooms_t,
                   tensors["room_results"], nr, C.byref(text) if text is not None else None, flags, tensors["jconns"],
                   tensors["want"], results_t, slot=dec.slot)
        return GroupRoster(self, bcast, room_set, tensors)

    def _backlog_row(self, row, t, k, bcast_row, replied, room=_lib.ROOM_NONE, flags=0):
        """Item k's xyws_backlog_conn row: its send tensor t behind what the
        row at bcast_row says was written, its reply row when the sweep has
        one, and the room it joins (BL_JOIN in flags) or none."""
        _set_out(row, t)
        row.bcast, row.reply = bcast_row, self._reply_row(k) if replied else 0
        row.room, row.flags = room, flags

    def state_tensors(self):
        """Every tensor of the group that carries state from one sweep to the
        next (the carries, the counts, the backlog's logs and carries)."""
        return [self.carry_t, self.rcarry_t, self.mcarry_t, self.hcarry_t, self.counts_t] + \
            [log for log, _ in self._blogs] + list(self._bcarries)

    def backlog_carry(self, room):
        """Host copy of a room's backlog carry (synchronizes)."""
        if not 0 <= room < len(self._bcarries):
            raise XywsError(-1, "no such room")
        return _lib.BacklogCarry.from_buffer_copy(self._bcarries[room].cpu().numpy().tobytes())

    def backlog_bytes(self, room):
        """The frames room `room` holds for its next joiner, oldest first (a device tensor; synchronizes)."""
        c = self.backlog_carry(room)
        return self._blogs[room][0][c.start:c.start + c.len]

    def backlog(self, bcast, joiners=None, keep=10, log_cap=None):
        """Keep each room's recent messages and send them to joiners
        (xyws_backlog_streams, at most two launches), after broadcast() of the
        same sweep: `bcast` is its GroupBroadcast. The sweep's newest frames
        are folded into each room's log on the device, `keep` of them at most
        (the reference keeps 10; 16 at most), and the log is appended to the
        send tensor of every joiner behind what broadcast() left there.
        joiners: (conn_id, room) pairs, or a dict; a joiner must be an item of
        this sweep, and the caller lists it in rooms[room] from the next
        sweep on. The group allocates a room's log (log_cap bytes, default
        2 * keep * 4096 + 30) and carry when the room is first seen and keeps
        them across sweeps: room r is the same room in every call, and a
        log_cap other than the one its log was made with is refused. When
        broadcast() was given the sweep's reply, a joiner whose reply closed
        or overflowed is sent nothing (XYWS_BLC_NOT_RECEIVER). Given the
        GroupRoster of the sweep in place of `bcast`, the joiners are the ones
        roster() admitted (marked on the device: pass none) and the backlog
        goes behind the notices. Returns a GroupBacklog. Call it before the
        group's next decode()."""
        import torch
        roster = bcast if isinstance(bcast, GroupRoster) else None
        if roster is not None:  # the joiners are the ones roster() admitted: its jconns table names them on the device
            if joiners:
                raise XywsError(-1, "after roster() the joiners are the roster's: pass none")
            bcast = roster.bcast
        if not isinstance(bcast, GroupBroadcast) or bcast.group is not self:
            raise XywsError(-1, "backlog() takes the result of this group's broadcast() or roster()")
        dec = bcast.decoded
        m, nr = len(dec.ids), len(bcast._wires)
        keep = int(keep)
        cap = 2 * max(min(keep, _lib.BACKLOG_MAX), 1) * 4096 + 30 if log_cap is None else int(log_cap)
        if keep < 0 or cap < 0:
            raise ValueError("keep and log_cap must not be negative")
        item = {i: k for k, i in enumerate(dec.ids)}
        pairs = list(joiners.items()) if isinstance(joiners, dict) else list(joiners or [])
        joined = {}
        for i, r in pairs:
            if int(i) not in item or int(i) in joined or not 0 <= int(r) < nr:
                raise XywsError(-1, "a joiner must be an item of this sweep, join once, and name a room of the sweep")
            joined[int(i)] = int(r)
        if log_cap is not None and any(lcap != cap for _, lcap in self._blogs[:nr]):
            raise XywsError(-1, "a room's log keeps the log_cap it was made with")
        while len(self._blogs) < nr:
            self._blogs.append((torch.empty(max(cap, 1), dtype=torch.uint8, device=self.device), cap))
            self._bcarries.append(_lib.alloc_rows(_lib.BacklogCarry, 1, self.device))
        rtab = _lib.Table(_lib.BacklogRoom, nr)
        for r in range(nr):
            row, (log, lcap) = rtab[r], self._blogs[r]
            row.log, row.log_cap, row.bc, row.keep = log.data_ptr(), lcap, self._bcarries[r].data_ptr(), keep
        jtab = _lib.Table(_lib.BacklogConn, m)
        for k, (row, i, t) in enumerate(zip(jtab.rows, dec.ids, bcast.outs)):
            # (the reply row broadcast() named: only it says that a joiner, not yet a member, closed or overflowed)
            room, fl = (joined[i], _lib.BL_JOIN) if i in joined else (_lib.ROOM_NONE, 0)
            self._backlog_row(row, t, k, _lib.row_ptr(bcast.results_t, _lib.BcastResult, k), bcast.replied, room, fl)
        tensors = dict(brooms=rtab.upload(self.device),
                       jconns=jtab.upload(self.device) if roster is None else roster.jconns_t,
                       room_results=_lib.alloc_rows(_lib.BacklogRoomResult, nr, self.device),
                       results=_lib.alloc_rows(_lib.BacklogResult, m, self.device))
        # (after roster() the room table holds the next sweep's lists: the fold walks the ones this sweep's
        # broadcast read, which roster() left in the room set's `seen` rows)
        rooms_t = bcast.rooms_t if roster is None else roster.room_set.seen_rooms_t
        self._call("xyws_backlog_streams", *bcast.messages.tables(), bcast.bconns_t, m, rooms_t, bcast.room_results_t,
                   tensors["brooms"], tensors["room_results"], nr, tensors["jconns"], tensors["results"],
                   slot=dec.slot)
        return GroupBacklog(self, bcast, roster, tensors, nr)

    def outbox(self, last, accept=None, pack_cap=None, host=False):
        """Pack what a sweep left to send (xyws_outbox_streams, three
        launches, the sweep's last call): `last` is the sweep's last result
        object, a GroupBacklog, GroupRoster, GroupBroadcast or GroupReply (None
        for a sweep of handshakes alone); accept, the GroupAccept of the sweep
        for the connections still in HTTP state. Row i of the table is item i
        of `last`, named by the rows the sweep's calls wrote for it; an
        accept() item that is an item of the sweep gives its row the accept
        row, any other gets a row of its own behind them. pack_cap: the pack's
        capacity (default: what always suffices). host=True puts the pack, the
        list and the summary into pinned host memory, which the kernels write
        through its device pointer (xyws_outbox_map). Returns a GroupOutbox."""
        import torch
        roster = bcast = reply = None
        backlog = last if isinstance(last, GroupBacklog) else None
        if backlog is not None:
            roster, bcast = backlog.roster, backlog.bcast
        elif isinstance(last, GroupRoster):
            roster, bcast = last, last.bcast
        elif isinstance(last, GroupBroadcast):
            bcast = last
        elif isinstance(last, GroupReply):
            reply = last
        elif last is not None or accept is None:
            raise XywsError(-1, "outbox() takes the result of this group's backlog(), roster(), broadcast() or reply()")
        if (last is not None and last.group is not self) or (accept is not None and accept.group is not self):
            raise XywsError(-1, "outbox() takes results of this group")
        if pack_cap is not None and int(pack_cap) < 0:
            raise ValueError("pack_cap must not be negative")
        ids = [] if last is None else list(last.decoded.ids)
        if bcast is not None:
            outs, replied = list(bcast.outs), bcast.replied
        else:
            outs, replied = (list(reply.outs), True) if reply is not None else ([], False)
        m = len(ids)
        item = {i: k for k, i in enumerate(ids)}
        acc_of = {}
        for j, i in enumerate(accept.ids if accept is not None else []):
            if i in item:
                acc_of[item[i]] = j
            else:
                acc_of[len(ids)] = j
                ids.append(i)
                outs.append(accept.outs[j])
        n = len(ids)
        tab = _lib.Table(_lib.OutboxConn, n)
        sent = roster if roster is not None else bcast  # (an xyws_roster_result reads as an xyws_bcast_result)
        for k, (row, t) in enumerate(zip(tab.rows, outs)):
            row.out, row.out_cap = (t.data_ptr(), t.numel()) if t.numel() else (0, 0)
            if k < m:
                row.backlog = _lib.row_ptr(backlog.results_t, _lib.BacklogResult, k) if backlog is not None else 0
                row.bcast = _lib.row_ptr(sent.results_t, _lib.BcastResult, k) if sent is not None else 0
                # (as roster(): a connection still in HTTP state has no reply row of this sweep)
                row.reply = self._reply_row(k) if replied and k not in acc_of else 0
            row.accept = _lib.row_ptr(accept.results_t, _lib.AcceptResult, acc_of[k]) if k in acc_of else 0
        cap = sum((t.numel() + 15) & ~15 for t in outs) if pack_cap is None else int(pack_cap)
        L = self.ctx.L
        where = "cpu" if host else self.device
        keep = dict(pack=torch.zeros(max(cap, 16), dtype=torch.uint8, device=where),
                    entries=_lib.alloc_rows(_lib.OutboxEntry, n, where),
                    summary=_lib.alloc_rows(_lib.OutboxSummary, 1, where))
        if host:
            ptr = {}
            with torch.cuda.device(self.device):
                keep = {k: t.pin_memory() for k, t in keep.items()}
                for k, t in keep.items():
                    d = C.c_void_p()
                    check(L.xyws_outbox_map(t.data_ptr(), C.byref(d)), "xyws_outbox_map")
                    ptr[k] = d.value
        else:
            ptr = {k: t.data_ptr() for k, t in keep.items()}
        tensors = dict(keep, conns=tab.upload(self.device),
                       scratch=torch.empty(max(L.xyws_outbox_scratch_bytes(n), 8), dtype=torch.uint8, device=self.device))
        done = _Done()
        self._call("xyws_outbox_streams", tensors["conns"], n, ptr["pack"] if cap else None, cap, ptr["entries"],
                   ptr["summary"], tensors["scratch"], tensors["scratch"].numel(), done=done)
        return GroupOutbox(self, ids, outs, tensors, cap, host, last, accept, done)

    def _inbox_state(self, recv_cap, resp_cap):
        """The receive slab, the inbox carries and the resident tables (made once)."""
        import torch
        if self._ib is not None:
            if (recv_cap, resp_cap) != (self._ib["recv_cap"], self._ib["resp_cap"]):
                raise XywsError(-1, "recv_cap and resp_cap are fixed by the group's first inbox() call")
            return self._ib
        n, dev = self.n, self.device
        with torch.cuda.device(dev):
            ib = dict(recv_cap=recv_cap, resp_cap=resp_cap,
                      slab=torch.zeros(max(n * recv_cap, 16), dtype=torch.uint8, device=dev),
                      resp=torch.zeros(max(n * resp_cap, 16), dtype=torch.uint8, device=dev),
                      carries=_lib.alloc_rows(_lib.InboxCarry, n, dev),
                      aresults=_lib.alloc_rows(_lib.AcceptResult, n, dev),
                      results=_lib.alloc_rows(_lib.InboxResult, n, dev))
            conns, aconns = _lib.Table(_lib.Conn, n), _lib.Table(_lib.AcceptConn, n)
            for i in range(n):
                c, a = conns[i], aconns[i]
                self._conn_row(c, ib["slab"].data_ptr() + recv_cap * i, 0, i)
                a.buf, a.len, a.out, a.out_cap = c.buf, 0, ib["resp"].data_ptr() + resp_cap * i, resp_cap
            ib["conns"], ib["aconns"] = conns.upload(dev), aconns.upload(dev)
            iconns = _lib.Table(_lib.InboxConn, n)
            for i in range(n):
                r = iconns[i]
                r.buf, r.cap = ib["slab"].data_ptr() + recv_cap * i, recv_cap
                r.carry = _lib.row_ptr(ib["carries"], _lib.InboxCarry, i)
                r.conn, r.aconn = _lib.row_ptr(ib["conns"], _lib.Conn, i), _lib.row_ptr(ib["aconns"], _lib.AcceptConn, i)
                r.aresult = _lib.row_ptr(ib["aresults"], _lib.AcceptResult, i)
            ib["iconns"] = iconns.upload(dev)
        self._ib = ib
        return ib

    def inbox(self, pack, entries, recv_cap, m_cap=None, resp_cap=144):
        """Scatter a sweep's received bytes to the connections
        (xyws_inbox_streams, five launches, the sweep's first call). pack: the
        received bytes, dense (bytes, or a uint8 tensor on the group's device);
        entries: one (conn, off, len, at[, flags]) tuple per completed recv in
        arrival order, `at` the connection's bytes in this sweep before it;
        recv_cap: the size of every connection's receive range. The first call
        makes the group's receive slab, inbox carries and the resident n-row
        xyws_conn and xyws_accept_conn tables; decode() and accept() take the
        returned GroupInbox in place of their item lists; the sweep's later
        calls (reply() .. outbox()) do not take what that decode() returns.
        reset(ids) before the call hands a slot to a new connection. m_cap: the
        entry capacity of the call (default len(entries))."""
        import numpy as np
        import torch
        recv_cap, resp_cap = int(recv_cap), int(resp_cap)
        if recv_cap < 1 or resp_cap < 0:
            raise XywsError(-1, "recv_cap must be positive and resp_cap not negative")
        ents = [tuple(int(v) for v in e) for e in entries]
        if any(len(e) not in (4, 5) or min(e) < 0 or e[0] > 0xFFFFFFFF for e in ents):
            raise XywsError(-1, "an entry is (conn, off, len, at[, flags]), none of them negative")
        m = len(ents)
        m_cap = m if m_cap is None else int(m_cap)
        if m_cap < m:
            raise XywsError(-1, "more entries than m_cap")
        if isinstance(pack, (bytes, bytearray, memoryview)):
            raw = bytes(pack)
            pack_t = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(self.device) if raw else None
        else:
            pack_t = _dev_u8(pack) if pack.numel() else None
            if pack_t is not None and pack_t.device != self.device:
                raise XywsError(-1, "a pack on another device than the group's")
        ib = self._inbox_state(recv_cap, resp_cap)
        pack_len = pack_t.numel() if pack_t is not None else 0
        L = self.ctx.L
        need = L.xyws_inbox_scratch_bytes(self.n, m_cap)
        head = _lib.Table(_lib.InboxHead, 1)
        head[0].m, head[0].pack_len = m, pack_len
        tab = _lib.Table(_lib.InboxEntry, m_cap)
        for row, e in zip(tab.rows, ents):
            row.conn, row.off, row.len, row.at, row.flags = e[0], e[1], e[2], e[3], e[4] if len(e) == 5 else 0
        tensors = dict(head=head.upload(self.device), entries=tab.upload(self.device), pack=pack_t,
                       summary=_lib.alloc_rows(_lib.InboxSummary, 1, self.device), results=ib["results"],
                       scratch=torch.empty(max(need, 8), dtype=torch.uint8, device=self.device))
        done = _Done()
        self._call("xyws_inbox_streams", ib["iconns"], self.n, tensors["head"], tensors["entries"] if m_cap else None,
                   m_cap, pack_t if pack_len else None, pack_len, ib["results"], tensors["summary"], tensors["scratch"],
                   tensors["scratch"].numel(), done=done)
        return GroupInbox(self, tensors, m, done)

    def inbox_carry(self, conn_id):
        """Host copy of a connection's inbox carry (synchronizes)."""
        if not 0 <= conn_id < self.n or self._ib is None:
            raise XywsError(-1, "no such connection, or no inbox() call yet")
        return self._carry_of(self._ib["carries"], _lib.InboxCarry, conn_id)

    def msg_carry(self, conn_id):
        """Host copy of a connection's message carry (synchronizes)."""
        return self._carry_of(self.mcarry_t, _lib.MsgCarry, conn_id)


def decode_indexed(buf, starts, frames=True, parse_only=False):
    """Frames at known offsets (ascending): parse + unmask in place."""
    import torch
    t = _dev_u8(buf)
    ctx = context(t.device.index)
    st = torch.as_tensor(starts, dtype=torch.int64).to(t.device)
    n = st.numel()
    frames_t = _lib.alloc_rows(Frame, n, t.device, zero=False) if frames else None
    check(ctx.L.xyws_decode_indexed(
        ctx.h, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(st.data_ptr()), n,
        C.c_void_p(frames_t.data_ptr()) if frames_t is not None else None,
        1 if parse_only else 0, _stream(t)), "xyws_decode_indexed")
    res = DecodeResult(frames_t, None, n)
    res.nframes_t = torch.tensor([n], dtype=torch.int64)
    return res


class websocket_frame_header_parser:
    """websocket_frame_header_parser (:226-385) through xyws_parser_* (C-ABI).

    parse(data) takes bytes (host) or a device uint8 tensor and returns the
    number of bytes consumed in THIS call up to the end of the header, or
    ``npos`` while the header is incomplete; once a header completed, further
    input returns npos until reset() (:378-384). result() returns (flags,
    mask_uint32_t, length) (websocket.h:121-128). The bytes are parsed on the
    device (stream decoder, parse-only, device-resident carry).
    """
    npos = npos

    def __init__(self, device=None):
        import torch
        self.ctx = context(device)
        self.L = self.ctx.L
        h = C.c_void_p()
        check(self.L.xyws_parser_create(self.ctx.h, C.byref(h)), "xyws_parser_create")
        self.h = h
        self._stream = C.c_void_p(torch.cuda.current_stream(self.ctx.device).cuda_stream)

    def __del__(self):
        try:
            if self.h:
                self.L.xyws_parser_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def reset(self):
        check(self.L.xyws_parser_reset(self.h), "xyws_parser_reset")

    def parse(self, data):
        import torch
        consumed = C.c_uint64()
        if isinstance(data, torch.Tensor):
            t = _dev_u8(data)
            ptr, n = C.c_void_p(t.data_ptr()), t.numel()
            check(self.L.xyws_parser_parse(self.h, ptr, n, C.byref(consumed), _stream(t)), "xyws_parser_parse")
        else:
            b = bytes(data)
            buf = C.create_string_buffer(b, max(len(b), 1))
            check(self.L.xyws_parser_parse(self.h, buf, len(b), C.byref(consumed), self._stream),
                  "xyws_parser_parse")
        return consumed.value

    def _res(self):
        f, ln = C.c_uint8(), C.c_uint64()
        key = (C.c_uint8 * 4)()
        check(self.L.xyws_parser_result(self.h, C.byref(f), key, C.byref(ln)), "xyws_parser_result")
        return websocket_flags(f.value), int.from_bytes(bytes(key), "little"), ln.value

    def flags(self):
        return self._res()[0]

    def length(self):
        return self._res()[2]

    def mask_uint32_t(self):
        return self._res()[1]

    def mask(self):
        return self._res()[1].to_bytes(4, "little")

    def result(self):
        return self._res()


# ---------------------------------------------------------------------------
# the callers either side of the decode path (xyws_frames.hip)

class websocket_request_handler:
    """class websocket_request_handler (websocket_request_handler.h:66-264)
    over xyws_accept_request: host bytes only, no context and no device (the
    kernel's grammar compiled for the host). parse() takes the accumulated
    request and returns what the reference's does: the bytes consumed, -1 for
    a grammar error, -2 while incomplete. generate_response() returns the 101
    or, as there, the bad-request response for whatever was not a whole valid
    request. The default policy is the reference's (ACC_REFERENCE); policy 0
    answers by RFC 6455 4.2.1."""

    def __init__(self, policy=_lib.ACC_REFERENCE, max_request=_lib.ACCEPT_MAX_REQUEST):
        self.L = _lib.load()
        self.policy, self.max_request = policy, max_request
        self._req, self._res, self._resp = b"", _lib.AcceptResult(), b""

    def _run(self, data):
        res, out = _lib.AcceptResult(), (C.c_uint8 * 144)()
        check(self.L.xyws_accept_request(data, len(data), self.max_request, self.policy, out, 144, C.byref(res)),
              "xyws_accept_request")
        return res, bytes(out[:res.resp_len])

    def parse(self, data):
        self._req = bytes(data)
        self._res, self._resp = self._run(self._req)
        if self._res.reason == _lib.ACR_PARSE:
            return -1
        return self._res.consumed if self._res.consumed else -2

    def generate_response(self):
        if not self._res.status & (_lib.ACC_ACCEPTED | _lib.ACC_REJECTED):
            self._resp = self._run(b"\x01")[1]  # not parsed (never, or incomplete): the handler's bad request
        return self._resp

    def response_view(self):
        return self._resp

    def get_path(self):
        return self._req[self._res.path_off:self._res.path_off + self._res.path_len]

    def get_room(self, table_bytes):
        """The room the request target goes to by the route table
        `table_bytes` (_lib.route_table's blob), None when no route matches
        (xyws_route_lookup: the kernel's lookup compiled for the host)."""
        path, res = self.get_path(), _lib.RouteResult()
        check(self.L.xyws_route_lookup(table_bytes, len(table_bytes), path, len(path), C.byref(res)), "xyws_route_lookup")
        return res.room if res.status & _lib.RT_MATCHED else None

    def result(self):
        return self._res


def _opt_ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def encode_frames(src, frames_t, n, flags, dev_n=None, enc_opts=0, keys=None, verdicts=None,
                  action_mask=0, out=None, offsets=None):
    """echo_once's replies for a decoded frame table, on the device
    (xyws_encode_frames). src: the decoded batch (device uint8); frames_t:
    n xyws_frame records (device uint8, n*32 bytes); keys: device uint8 (4 per
    frame) for client-role masking. Returns (out, out_len tensor)."""
    import torch
    t = _dev_u8(src)
    ctx = context(t.device.index)
    olen = torch.zeros(1, dtype=torch.int64, device=t.device)
    if out is None:
        raise XywsError(-1, "encode_frames needs an output tensor (size it with encode_size)")
    check(ctx.L.xyws_encode_frames(ctx.h, C.c_void_p(t.data_ptr()), t.numel(), _opt_ptr(frames_t), n,
                                   _opt_ptr(dev_n), int(flags) & 0xFF, enc_opts, _opt_ptr(keys),
                                   _opt_ptr(verdicts), action_mask, C.c_void_p(out.data_ptr()), out.numel(),
                                   _opt_ptr(offsets), C.c_void_p(olen.data_ptr()), _stream(t)),
          "xyws_encode_frames")
    return out, olen


def classify_frames(src, frames_t, n, max_payload, policy=0, dev_n=None, verdicts=None):
    """websocket_check_parser_result per frame (xyws_classify_frames): returns
    (verdicts tensor (n*8 bytes), first-close tensor). verdicts: the caller's
    device uint8 tensor for the records (n*8 bytes at least) instead of a
    fresh zeroed one."""
    import torch
    t = _dev_u8(src)
    ctx = context(t.device.index)
    if verdicts is None:
        verd = _lib.alloc_rows(_lib.Verdict, n, t.device)
    else:
        verd = _dev_u8(verdicts)
        if verd.numel() < n * C.sizeof(_lib.Verdict):
            raise XywsError(-1, "verdicts tensor smaller than n records")
    first = torch.zeros(1, dtype=torch.int64, device=t.device)
    check(ctx.L.xyws_classify_frames(ctx.h, C.c_void_p(t.data_ptr()), t.numel(), _opt_ptr(frames_t), n,
                                     _opt_ptr(dev_n), max_payload, policy, C.c_void_p(verd.data_ptr()),
                                     C.c_void_p(first.data_ptr()), _stream(t)), "xyws_classify_frames")
    return verd, first


def _out_and_msgs(t, out, out_cap, msgs, msg_cap, records):
    """The out tensor and the record tensor of a reassembly of the batch t,
    each with its capacity: the caller's, checked against out_cap / msg_cap,
    or a fresh zeroed one (as many bytes as t by default, and `records`
    records). Returns (out, out_cap, msgs, msg_cap)."""
    import torch
    size = C.sizeof(_lib.Message)
    if out is not None:
        out = _dev_u8(out)
        cap = out.numel() if out_cap is None else out_cap
        if cap > out.numel():
            raise XywsError(-1, "out_cap exceeds the out tensor")
    else:
        cap = t.numel() if out_cap is None else out_cap
        out = torch.zeros(max(cap, 1), dtype=torch.uint8, device=t.device)
    if msgs is not None:
        msgs = _dev_u8(msgs)
        mcap = msgs.numel() // size if msg_cap is None else msg_cap
        if mcap * size > msgs.numel():
            raise XywsError(-1, "msg_cap exceeds the msgs tensor")
    else:
        mcap = records if msg_cap is None else msg_cap
        msgs = _lib.alloc_rows(_lib.Message, mcap, t.device)
    return out, cap, msgs, mcap


def reassemble(src, frames_t, n, opts=0, out_cap=None, msg_cap=None, dev_n=None, out=None, msgs=None):
    """FIN=0 chains gathered into messages (xyws_reassemble): returns (out,
    messages tensor (msg_cap records), count tensor). out / msgs: the
    caller's device uint8 tensors (out_cap defaults to out's size, msg_cap to
    the records msgs holds) instead of fresh zeroed ones."""
    import torch
    t = _dev_u8(src)
    ctx = context(t.device.index)
    out, cap, msgs, mcap = _out_and_msgs(t, out, out_cap, msgs, msg_cap, max(n, 1))
    cnt = torch.zeros(1, dtype=torch.int64, device=t.device)
    check(ctx.L.xyws_reassemble(ctx.h, C.c_void_p(t.data_ptr()), t.numel(), _opt_ptr(frames_t), n, _opt_ptr(dev_n),
                                opts, C.c_void_p(out.data_ptr()), cap, C.c_void_p(msgs.data_ptr()), mcap,
                                C.c_void_p(cnt.data_ptr()), _stream(t)), "xyws_reassemble")
    return out, msgs, cnt


class message_assembler:
    """xyws_reassemble across batch boundaries (xyws_reassemble_stream): holds
    the device-resident xyws_msg_carry of one connection, as frame_decoder
    holds its xyws_carry. feed() takes each batch frame_decoder.decode()
    decoded, with that call's frame table, in order."""

    def __init__(self, device=None, opts=_lib.REASM_UTF8, ctx=None):
        import torch
        self.ctx = ctx if ctx is not None else context(device)
        self.device = torch.device("cuda", self.ctx.device)
        self.carry_t = _lib.alloc_rows(_lib.MsgCarry, 1, self.device)
        self.opts = opts

    def reset(self):
        self.carry_t.zero_()

    def carry(self):
        """Host copy of the carry (synchronizes)."""
        return _lib.read_rows(_lib.MsgCarry, self.carry_t, 1)[0]

    def feed(self, src, frames_t, n, dev_n=None, out=None, msgs=None, out_cap=None, msg_cap=None):
        """One batch: returns (out, messages tensor (msg_cap records), count
        tensor) like reassemble(); record 0 continues the message the last
        batch left open (MSG_CONTINUED). msg_cap defaults to n + 1 records."""
        import torch
        t = _dev_u8(src)
        out, cap, msgs, mcap = _out_and_msgs(t, out, out_cap, msgs, msg_cap, n + 1)
        cnt = torch.zeros(1, dtype=torch.int64, device=t.device)
        cp = C.c_void_p(self.carry_t.data_ptr())
        check(self.ctx.L.xyws_reassemble_stream(
            self.ctx.h, C.c_void_p(t.data_ptr()), t.numel(), _opt_ptr(frames_t), n, _opt_ptr(dev_n), self.opts,
            cp, cp, C.c_void_p(out.data_ptr()), cap, C.c_void_p(msgs.data_ptr()), mcap,
            C.c_void_p(cnt.data_ptr()), _stream(t)), "xyws_reassemble_stream")
        return out, msgs, cnt


class RecvArena:
    """A connection's receive arena (xyws_arena_*): recv into pinned host
    memory, decode on the device with the connection's carry, results and the
    unmasked bytes back in place; each completion writes 1 to `eventfd` (the
    fd an io_uring loop keeps a poll_add on, io_service.h:362-381)."""

    def __init__(self, nbytes, max_frames, eventfd=-1, device=None, host=None):
        self.ctx = context(device)
        self.L = self.ctx.L
        h = C.c_void_p()
        check(self.L.xyws_arena_create(self.ctx.h, host, nbytes, max_frames, eventfd, C.byref(h)),
              "xyws_arena_create")
        self.h = h
        self.nbytes = nbytes
        self.max_frames = max_frames
        self.host_ptr = self.L.xyws_arena_host(h)

    def view(self):
        """The receive area as a writable memoryview (pinned host memory)."""
        return (C.c_uint8 * self.nbytes).from_address(self.host_ptr)

    def submit(self, offset, length, opts=0):
        seq = C.c_uint64()
        rc = self.L.xyws_arena_submit(self.h, offset, length, opts, C.byref(seq))
        if rc == _lib.XYWS_ERR_AGAIN:
            return None
        check(rc, "xyws_arena_submit")
        return seq.value

    def poll(self, seq):
        res = _lib.ArenaResult()
        rc = self.L.xyws_arena_poll(self.h, seq, C.byref(res))
        if rc == _lib.XYWS_ERR_AGAIN:
            return None
        check(rc, "xyws_arena_poll")
        return res

    def wait(self, seq):
        res = _lib.ArenaResult()
        check(self.L.xyws_arena_wait(self.h, seq, C.byref(res)), "xyws_arena_wait")
        return res

    @staticmethod
    def frames_of(res, max_frames):
        return [res.frames[i] for i in range(min(res.nframes, max_frames))]

    def close(self):
        if getattr(self, "h", None):
            self.L.xyws_arena_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_plan(batch, n_shards, carry=None):
    """Cut one batch of back-to-back frames (host bytes: bytes, bytearray,
    numpy uint8 array, or a CPU uint8 tensor) into n_shards byte ranges at
    frame boundaries, balanced by bytes (xyws_shard_plan). Returns the
    n_shards + 1 bounds; shard k is batch[bounds[k]:bounds[k+1]], shard 0
    continues from `carry` (a Carry or None), the others start fresh."""
    import numpy as np
    L = _lib.load()
    if hasattr(batch, "numpy"):
        batch = batch.numpy()
    arr = np.ascontiguousarray(np.frombuffer(batch, dtype=np.uint8) if isinstance(batch, (bytes, bytearray))
                               else batch, dtype=np.uint8)
    out = (C.c_uint64 * (n_shards + 1))()
    cin = C.byref(carry) if carry is not None else None
    check(L.xyws_shard_plan(C.c_void_p(arr.ctypes.data) if arr.size else None, arr.size, cin, int(n_shards), out),
          "xyws_shard_plan")
    return list(out)


def shard_plan_frames(frames, length, n_shards):
    """shard_plan from a host frame table (a sequence of Frame, or a ctypes
    Frame array), frame_off ascending (xyws_shard_plan_frames)."""
    L = _lib.load()
    n = len(frames)
    arr = frames if isinstance(frames, C.Array) else \
        (Frame * max(n, 1)).from_buffer_copy(b"".join(bytes(f) for f in frames).ljust(C.sizeof(Frame) * max(n, 1), b"\0"))
    out = (C.c_uint64 * (n_shards + 1))()
    check(L.xyws_shard_plan_frames(arr, n, int(length), int(n_shards), out), "xyws_shard_plan_frames")
    return list(out)
