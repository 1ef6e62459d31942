"""ctypes binding of libxyws.so (include/xyws.h) and libxyws_tools.so.

The decode path has no CPU fallback: if the in-tree HIP library is missing or a
device is absent, calls raise XywsError instead of computing anything on the
host.
"""
import ctypes as C
import os
import re

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
HEADER = os.path.join(ROOT, "include", "xyws.h")

XYWS_OK = 0
XYWS_ERR_DEVICE = -5
# Every XYWS_OPT_* bit under its header's name, by value: the only Python list
# (tests/test_opts.py holds it to the headers). include/xyws.h:
OPT_PARSE_ONLY = 0x1
OPT_UNMASKED_HINT = 0x2
OPT_SERIAL_SCAN = 0x4
# internal (xynet_amd/csrc/xyws_stream.h, where each is described):
OPT_WG256 = 0x8
OPT_TEST_LATSPEC = 0x10
OPT_TEST_LATDUMP = 0x20
OPT_LATX_NOWORK = 0x40
OPT_LATX_ONLY = 0x80
OPT_STATS = 0x100
OPT_SMALL_SEG = 0x200
OPT_LATTICE = 0x400
OPT_NO_LATDEC = 0x800
OPT_NO_DENSE0 = 0x1000
OPT_REDIRECT = 0x2000
OPT_NO_LATENTRY = 0x4000
OPT_WG1024 = 0x8000
OPT_RUNS_NOWAIT = 0x10000
OPT_NO_STORE = 0x20000
OPT_WG512 = 0x40000
OPT_DIAG = 0x80000
OPT_TEST_GIVEUP = 0x100000
OPT_NO_LATTICE = 0x200000
OPT_STEAL = 0x400000
OPT_TEST_STEAL = 0x800000
OPT_LAT_NOGATE = 0x1000000
OPT_LAT_GATE = 0x2000000
OPT_BIGSCAN = 0x4000000
OPT_LATX_NOCHK = 0x8000000
OPT_IOV_PIECES = 0x10000000
OPT_IOV_STAGE = 0x20000000
OPT_NO_BIGSCAN = 0x40000000
OPT_RUNS = 0x80000000
# The scratch layout section of xynet_amd/csrc/xyws_stream.h (where each is
# described), under the header's names, by value: tests/test_layout.py holds
# every one to the header. Debug stats slots (xyws_debug_stats: NSTATS words),
# the run decoder's:
NSTATS = 48  # XYWS_NSTATS
ST_RUNS, ST_NONE, ST_BAD, ST_REPAIR, ST_CUT, ST_SPIN, ST_SEGS, ST_FRAMES = 0, 1, 2, 3, 4, 5, 6, 7
ST_P_WIN, ST_P_CAND, ST_P_UND, ST_P_TCOMP, ST_P_TCHECK, ST_P_TRES = 8, 9, 10, 11, 12, 13
ST_D_TENT, ST_D_TCHASE = 14, 15
ST_T_PRO, ST_T_MAIN, ST_T_WAIT, ST_T_FILL, ST_T_CHASE, ST_T_XOR = 16, 17, 18, 19, 20, 21
ST_T_TAIL, ST_T_PF, ST_T_CP = 22, 23, 24
ST_P_FILL, ST_P_SCAN, ST_P_PUB, ST_D_NOENT, ST_D_CHASE, ST_D_MISMATCH, ST_D_OVF = 25, 26, 27, 28, 29, 30, 31
ST_GIVEUP, ST_BRIDGE, ST_STEAL_REQ, ST_STEAL_ACC, ST_STEAL_SEGS = 32, 33, 34, 35, 36
ST_D_TVAL, ST_T_ROWS, ST_T_SER = 37, 38, 39
ST_P_LATTICE, ST_X_W0, ST_X_BITS, ST_X_SURV, ST_T_STRIDE = 40, 41, 42, 43, 46
# ...and the lattice decoder's (it shares slots 16..29 with the run decoder's timing slots)
LT_C_A, LT_C_C, LT_C_ADV, LT_D_FILL, LT_D_WB, LT_D_TAB, LT_D_WC = 16, 17, 18, 19, 20, 21, 22
LT_D_MASK, LT_D_WD, LT_D_ST, LT_D_WA, LT_SEGS, LT_GATE, LT_END = 23, 24, 25, 26, 27, 28, 29
# run record words (xyws_debug_records: R_WORDS u64 per flat index)
R_WORDS = 32
R_H, R_W, R_S0, R_HEAD, R_OKW, R_HN, R_WN, R_CNT, R_TAIL, R_FIRST, R_F0 = 0, 1, 2, 7, 8, 9, 10, 11, 12, 13, 14
R_EFROM, R_ECNT, R_EORD, R_ECARRY, R_EP = 20, 21, 22, 23, 24
R_T0, R_T1, R_T2, R_SPLIT, R_XCC, R_NREC = 25, 26, 27, 28, 29, 30
# pinned policy words (xyws_debug_policy, xyws_debug_plan: POL_WORDS u64) and the decoder codes in POL_DECODER
POL_EPOCH, POL_BYTES, POL_FSMIN, POL_FSMAX, POL_DECODER, POL_WORDS = 0, 1, 2, 3, 4, 5
DEC_RUNS, DEC_RUNS512, DEC_LATTICE = 0, 2, 3
# device error bits (xyws_ctx_last_device_error)
DERR_TABLE, DERR_TIMEOUT, DERR_STALE, DERR_TAG, DERR_SRC_OOB, DERR_ORPHANS = 0x1, 0x2, 0x4, 0x8, 0x100, 0x200
ERRORS = {-1: "invalid argument", -2: "HIP runtime error", -3: "device allocation failed",
          -4: "scratch capacity exceeded", -5: "device-side error", -6: "not complete yet"}


class XywsError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"xyws error {code} ({ERRORS.get(code, '?')}){': ' + what if what else ''}")


class Frame(C.Structure):
    """xyws_frame (include/xyws.h), 32 bytes."""
    _fields_ = [("frame_off", C.c_int64), ("payload_off", C.c_int64),
                ("payload_len", C.c_uint64), ("key", C.c_uint8 * 4),
                ("flags", C.c_uint8), ("hdr_len", C.c_uint8),
                ("status", C.c_uint8), ("reserved", C.c_uint8)]


class Carry(C.Structure):
    """xyws_carry (include/xyws.h), 64 bytes."""
    _fields_ = [("payload_remaining", C.c_uint64), ("phase", C.c_uint64),
                ("frames_total", C.c_uint64), ("key", C.c_uint8 * 4),
                ("hdr_len", C.c_uint8), ("hdr", C.c_uint8 * 14),
                ("reserved", C.c_uint8 * 21)]


class Verdict(C.Structure):
    """xyws_verdict (include/xyws.h), 8 bytes."""
    _fields_ = [("close_code", C.c_uint16), ("peer_code", C.c_uint16), ("action", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


class Message(C.Structure):
    """xyws_message (include/xyws.h), 40 bytes."""
    _fields_ = [("first_frame", C.c_uint64), ("nframes", C.c_uint64), ("out_off", C.c_uint64),
                ("length", C.c_uint64), ("status", C.c_uint32), ("opcode", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


class MsgCarry(C.Structure):
    """xyws_msg_carry (include/xyws.h), 64 bytes."""
    _fields_ = [("length", C.c_uint64), ("nframes", C.c_uint64), ("first_frame", C.c_uint64),
                ("frame_remaining", C.c_uint64), ("frames_seen", C.c_uint64), ("status", C.c_uint32),
                ("opcode", C.c_uint8), ("frame_member", C.c_uint8), ("utf8_len", C.c_uint8),
                ("utf8", C.c_uint8 * 3), ("reserved", C.c_uint8 * 14)]


class ArenaResult(C.Structure):
    """xyws_arena_result (include/xyws.h)."""
    _fields_ = [("seq", C.c_uint64), ("offset", C.c_uint64), ("len", C.c_uint64), ("nframes", C.c_uint64),
                ("frames", C.POINTER(Frame)), ("carry", Carry)]


class Conn(C.Structure):
    """xyws_conn (include/xyws.h), 64 bytes: one connection's entry of an
    xyws_decode_streams table (every pointer a device address)."""
    _fields_ = [("buf", C.c_void_p), ("len", C.c_uint64), ("carry", C.c_void_p), ("frames", C.c_void_p),
                ("cap", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class ReplyCarry(C.Structure):
    """xyws_reply_carry (include/xyws.h), 32 bytes: one connection's state between xyws_reply_streams calls."""
    _fields_ = [("frame_remaining", C.c_uint64), ("frames_seen", C.c_uint64), ("replies_total", C.c_uint64),
                ("close_code", C.c_uint16), ("echoing", C.c_uint8), ("status", C.c_uint8),
                ("reserved", C.c_uint8 * 4)]


class ReplyConn(C.Structure):
    """xyws_reply_conn (include/xyws.h), 32 bytes: entry i goes with entry i of the xyws_conn table."""
    _fields_ = [("out", C.c_void_p), ("out_cap", C.c_uint64), ("rc", C.c_void_p), ("verdicts", C.c_void_p)]


class ReplyResult(C.Structure):
    """xyws_reply_result (include/xyws.h), 32 bytes."""
    _fields_ = [("reply_len", C.c_uint64), ("first_close", C.c_uint64), ("answered", C.c_uint32),
                ("close_code", C.c_uint16), ("status", C.c_uint16), ("reserved", C.c_uint64)]


assert C.sizeof(Frame) == 32 and C.sizeof(Carry) == 64 and C.sizeof(Conn) == 64
class ReasmConn(C.Structure):
    """xyws_reasm_conn (include/xyws.h), 64 bytes: entry i goes with entry i of the xyws_conn table."""
    _fields_ = [("out", C.c_void_p), ("out_cap", C.c_uint64), ("mc", C.c_void_p), ("msgs", C.c_void_p),
                ("msg_cap", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class ReasmResult(C.Structure):
    """xyws_reasm_result (include/xyws.h), 32 bytes."""
    _fields_ = [("out_len", C.c_uint64), ("nmsgs", C.c_uint64), ("completed", C.c_uint32),
                ("status", C.c_uint32), ("reserved", C.c_uint64)]


assert C.sizeof(ReplyCarry) == 32 and C.sizeof(ReplyConn) == 32 and C.sizeof(ReplyResult) == 32
assert C.sizeof(ReasmConn) == 64 and C.sizeof(ReasmResult) == 32


class Room(C.Structure):
    """xyws_room (include/xyws.h), 32 bytes: one room of an xyws_broadcast_streams call."""
    _fields_ = [("members", C.c_void_p), ("n_members", C.c_uint64), ("wire", C.c_void_p), ("wire_cap", C.c_uint64)]


class RoomResult(C.Structure):
    """xyws_room_result (include/xyws.h), 32 bytes."""
    _fields_ = [("wire_len", C.c_uint64), ("nmsgs", C.c_uint32), ("skipped", C.c_uint32),
                ("receivers", C.c_uint32), ("status", C.c_uint32), ("reserved", C.c_uint64)]


class BcastConn(C.Structure):
    """xyws_bcast_conn (include/xyws.h), 64 bytes: entry i goes with entry i of the xyws_reasm_conn table."""
    _fields_ = [("head", C.c_void_p), ("head_len", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_uint64),
                ("reply", C.c_void_p), ("room", C.c_uint32), ("reserved0", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class BcastResult(C.Structure):
    """xyws_bcast_result (include/xyws.h), 32 bytes."""
    _fields_ = [("send_len", C.c_uint64), ("bcast_len", C.c_uint64), ("status", C.c_uint32),
                ("reserved0", C.c_uint32), ("reserved", C.c_uint64)]


assert C.sizeof(Room) == 32 and C.sizeof(RoomResult) == 32 and C.sizeof(BcastConn) == 64
assert C.sizeof(BcastResult) == 32
ROOM_NONE = 0xFFFFFFFF
ROOM_TRUNCATED, ROOM_BAD_MEMBER, ROOM_MSG_CAP = 0x1, 0x2, 0x4  # xyws_room_result.status
BC_TRUNCATED, BC_NOT_RECEIVER, BC_NO_ROOM = 0x1, 0x2, 0x4  # xyws_bcast_result.status


class HoldCarry(C.Structure):
    """xyws_hold_carry (include/xyws.h), 32 bytes: one connection's state between xyws_hold_streams calls."""
    _fields_ = [("start", C.c_uint64), ("held", C.c_uint64), ("nframes", C.c_uint64), ("status", C.c_uint32),
                ("opcode", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class HoldConn(C.Structure):
    """xyws_hold_conn (include/xyws.h), 32 bytes: entry i goes with entry i of the xyws_reasm_conn table."""
    _fields_ = [("hold_cap", C.c_uint64), ("hc", C.c_void_p), ("vmsgs", C.c_void_p), ("vmsg_cap", C.c_uint64)]


class HoldResult(C.Structure):
    """xyws_hold_result (include/xyws.h), 32 bytes."""
    _fields_ = [("held", C.c_uint64), ("delivered_len", C.c_uint64), ("status", C.c_uint32),
                ("reserved0", C.c_uint32), ("reserved", C.c_uint64)]


assert C.sizeof(HoldCarry) == 32 and C.sizeof(HoldConn) == 32 and C.sizeof(HoldResult) == 32
HOLD_DELIVERED, HOLD_ACTIVE, HOLD_LOST, HOLD_DROPPED, HOLD_TOO_LONG, HOLD_PASSTHROUGH = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20


BACKLOG_MAX = 16


class BacklogCarry(C.Structure):
    """xyws_backlog_carry (include/xyws.h), 192 bytes: one room's state between xyws_backlog_streams calls."""
    _fields_ = [("start", C.c_uint64), ("len", C.c_uint64), ("count", C.c_uint32), ("gaps", C.c_uint32),
                ("total", C.c_uint64), ("flen", C.c_uint64 * BACKLOG_MAX), ("reserved", C.c_uint64 * 4)]


class BacklogRoom(C.Structure):
    """xyws_backlog_room (include/xyws.h), 32 bytes: entry r goes with entry r of the xyws_room table."""
    _fields_ = [("log", C.c_void_p), ("log_cap", C.c_uint64), ("bc", C.c_void_p), ("keep", C.c_uint32),
                ("reserved0", C.c_uint32)]


class BacklogRoomResult(C.Structure):
    """xyws_backlog_room_result (include/xyws.h), 32 bytes."""
    _fields_ = [("len", C.c_uint64), ("count", C.c_uint32), ("folded", C.c_uint32), ("dropped", C.c_uint32),
                ("status", C.c_uint32), ("reserved", C.c_uint64)]


class BacklogConn(C.Structure):
    """xyws_backlog_conn (include/xyws.h), 64 bytes: entry i goes with entry i of the xyws_bcast_conn table."""
    _fields_ = [("out", C.c_void_p), ("out_cap", C.c_uint64), ("bcast", C.c_void_p), ("reply", C.c_void_p),
                ("room", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64 * 3)]


class BacklogResult(C.Structure):
    """xyws_backlog_result (include/xyws.h), 32 bytes."""
    _fields_ = [("send_len", C.c_uint64), ("backlog_len", C.c_uint64), ("status", C.c_uint32),
                ("reserved0", C.c_uint32), ("reserved", C.c_uint64)]


assert C.sizeof(BacklogCarry) == 192 and C.sizeof(BacklogRoom) == 32 and C.sizeof(BacklogRoomResult) == 32
assert C.sizeof(BacklogConn) == 64 and C.sizeof(BacklogResult) == 32
BL_PASSTHROUGH, BL_BAD_CARRY, BL_MISMATCH, BL_GAP, BL_EVICTED, BL_TOO_LONG = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
BL_JOIN = 0x1  # xyws_backlog_conn.flags
BLC_JOINED, BLC_TRUNCATED, BLC_NO_ROOM, BLC_NOT_RECEIVER = 0x1, 0x2, 0x4, 0x8  # xyws_backlog_result.status
ROSTER_NAME_MAX, ROSTER_TEXT_MAX = 256, 32


class RosterConn(C.Structure):
    """xyws_roster_conn (include/xyws.h), 64 bytes: entry i goes with entry i of the xyws_bcast_conn table."""
    _fields_ = [("name", C.c_void_p), ("name_len", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_uint64),
                ("bcast", C.c_void_p), ("reply", C.c_void_p), ("accept", C.c_void_p), ("room", C.c_uint32),
                ("flags", C.c_uint32)]


class RosterRoom(C.Structure):
    """xyws_roster_room (include/xyws.h), 32 bytes: entry r goes with entry r of the xyws_room table."""
    _fields_ = [("member_cap", C.c_uint64), ("notes", C.c_void_p), ("notes_cap", C.c_uint64), ("seen", C.c_void_p)]


class RosterRoomResult(C.Structure):
    """xyws_roster_room_result (include/xyws.h), 32 bytes."""
    _fields_ = [("notes_len", C.c_uint64), ("welcome_off", C.c_uint64), ("joined", C.c_uint32), ("left", C.c_uint32),
                ("n_members", C.c_uint32), ("status", C.c_uint32)]


class RosterResult(C.Structure):
    """xyws_roster_result (include/xyws.h), 32 bytes: readable as an xyws_bcast_result."""
    _fields_ = [("send_len", C.c_uint64), ("note_len", C.c_uint64), ("status", C.c_uint32), ("room", C.c_uint32),
                ("note_off", C.c_uint64)]


class RosterText(C.Structure):
    """xyws_roster_text (include/xyws.h), 104 bytes, host memory: the strings of a notice."""
    _fields_ = [("head", C.c_uint8 * ROSTER_TEXT_MAX), ("joined", C.c_uint8 * ROSTER_TEXT_MAX),
                ("left", C.c_uint8 * ROSTER_TEXT_MAX), ("head_len", C.c_uint8), ("joined_len", C.c_uint8),
                ("left_len", C.c_uint8), ("reserved", C.c_uint8 * 5)]


assert C.sizeof(RosterConn) == 64 and C.sizeof(RosterRoom) == 32 and C.sizeof(RosterRoomResult) == 32
assert C.sizeof(RosterResult) == 32 and C.sizeof(RosterText) == 104
RS_JOIN, RS_LEAVE, RS_JOIN_ON_ACCEPT, RS_LEAVE_ON_CLOSE = 0x1, 0x2, 0x4, 0x8  # xyws_roster_conn.flags
RS_TRUNCATED, RS_FULL, RS_BAD_MEMBER = 0x10, 0x20, 0x40  # xyws_roster_room_result.status
(RSC_TRUNCATED, RSC_NOT_RECEIVER, RSC_NO_ROOM, RSC_MEMBER, RSC_JOINED, RSC_LEFT, RSC_FULL, RSC_ALREADY,
 RSC_BAD_NAME) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100  # xyws_roster_result.status
assert C.sizeof(ArenaResult) == 104
XYWS_ERR_AGAIN = -6
ARENA_SLOTS = 8
assert C.sizeof(Verdict) == 8 and C.sizeof(Message) == 40 and C.sizeof(MsgCarry) == 64
NPOS = (1 << 64) - 1
ENC_FRAME_OPCODE = 0x1
ACT_DATA, ACT_PING, ACT_PONG, ACT_CLOSE = 0, 1, 2, 3
POL_FRAGMENTS, POL_UNMASKED, POL_STRICT = 0x1, 0x2, 0x4
POL_REFERENCE = 0x8
RPL_TRUNCATED, RPL_CLOSED, RPL_OVERFLOW = 0x1, 0x2, 0x4  # xyws_reply_result.status
REASM_UTF8 = 0x1
MSG_COMPLETE, MSG_UTF8_BAD, MSG_INTERRUPTED, MSG_TRUNCATED, MSG_ORPHANS = 0x1, 0x2, 0x4, 0x8, 0x10
MSG_CONTINUED, MSG_UNCHECKED = 0x20, 0x40  # xyws_reassemble_stream only
MSG_OVERFLOW = 0x80  # xyws_msg_carry.status, xyws_reassemble_streams only
RSM_TRUNCATED, RSM_MSG_CAP, RSM_OVERFLOW, RSM_OPEN, RSM_UTF8_BAD = 0x1, 0x2, 0x4, 0x8, 0x10  # xyws_reasm_result.status


class AcceptConn(C.Structure):
    """xyws_accept_conn (include/xyws.h), 32 bytes: one connection still in HTTP state."""
    _fields_ = [("buf", C.c_void_p), ("len", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_uint64)]


class AcceptResult(C.Structure):
    """xyws_accept_result (include/xyws.h), 32 bytes."""
    _fields_ = [("status", C.c_uint32), ("http_status", C.c_uint16), ("reason", C.c_uint16),
                ("consumed", C.c_uint32), ("resp_len", C.c_uint32), ("path_off", C.c_uint32),
                ("path_len", C.c_uint32), ("key_off", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(AcceptConn) == 32 and C.sizeof(AcceptResult) == 32
ACCEPT_MAX_REQUEST = 8192
ACC_ACCEPTED, ACC_REJECTED, ACC_TRUNCATED = 0x1, 0x2, 0x4  # xyws_accept_result.status
ACC_REFERENCE = 0x100  # xyws_accept_streams policy
(ACR_NONE, ACR_PARSE, ACR_TOO_LONG, ACR_METHOD, ACR_VERSION, ACR_FOLDED, ACR_HOST, ACR_UPGRADE, ACR_CONNECTION,
 ACR_KEY, ACR_WS_VERSION) = range(11)  # xyws_accept_result.reason
ACR_NOT_FOUND = 11  # after xyws_route_streams' 404


class Route(C.Structure):
    """xyws_route (include/xyws.h), 24 bytes, host memory: one route given to xyws_route_build."""
    _fields_ = [("key", C.c_void_p), ("key_len", C.c_uint32), ("room", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class RouteConn(C.Structure):
    """xyws_route_conn (include/xyws.h), 8 bytes: entry k goes with entry k of the accept tables."""
    _fields_ = [("rconn", C.c_uint32), ("reserved", C.c_uint32)]


class RouteResult(C.Structure):
    """xyws_route_result (include/xyws.h), 32 bytes."""
    _fields_ = [("status", C.c_uint32), ("room", C.c_uint32), ("route", C.c_uint32), ("key_off", C.c_uint32),
                ("key_len", C.c_uint32), ("reserved", C.c_uint32 * 3)]


assert C.sizeof(Route) == 24 and C.sizeof(RouteConn) == 8 and C.sizeof(RouteResult) == 32
ROUTE_KEY_MAX, ROUTE_PREFIX, ROUTE_NO_ROW = 256, 0x1, 0xFFFFFFFF
RT_MISS_404 = 0x1  # xyws_route_streams policy
(RT_MATCHED, RT_BY_PREFIX, RT_MISS, RT_NOT_FOUND, RT_NOT_ACCEPTED, RT_BAD_ROW,
 RT_BAD_TABLE) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40  # xyws_route_result.status


class OutboxConn(C.Structure):
    """xyws_outbox_conn (include/xyws.h), 64 bytes: entry i is connection i of the sweep's tables."""
    _fields_ = [("out", C.c_void_p), ("out_cap", C.c_uint64), ("backlog", C.c_void_p), ("bcast", C.c_void_p),
                ("reply", C.c_void_p), ("accept", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class OutboxEntry(C.Structure):
    """xyws_outbox_entry (include/xyws.h), 32 bytes: one connection that sends or is closed."""
    _fields_ = [("conn", C.c_uint32), ("flags", C.c_uint32), ("off", C.c_uint64), ("len", C.c_uint64),
                ("full_len", C.c_uint64)]


class OutboxSummary(C.Structure):
    """xyws_outbox_summary (include/xyws.h), 64 bytes."""
    _fields_ = [("n_entries", C.c_uint64), ("pack_len", C.c_uint64), ("packed_len", C.c_uint64),
                ("send_bytes", C.c_uint64), ("n_close", C.c_uint32), ("n_truncated", C.c_uint32),
                ("n_deferred", C.c_uint32), ("status", C.c_uint32), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(OutboxConn) == 64 and C.sizeof(OutboxEntry) == 32 and C.sizeof(OutboxSummary) == 64
OB_CLOSE, OB_OVERFLOW, OB_TRUNCATED, OB_DEFERRED = 0x1, 0x2, 0x4, 0x8  # xyws_outbox_entry.flags
OBS_DEFERRED, OBS_TRUNCATED = 0x1, 0x2  # xyws_outbox_summary.status


class InboxHead(C.Structure):
    """xyws_inbox_head (include/xyws.h), 32 bytes: how many entries a sweep brought."""
    _fields_ = [("m", C.c_uint64), ("pack_len", C.c_uint64), ("reserved", C.c_uint64 * 2)]


class InboxEntry(C.Structure):
    """xyws_inbox_entry (include/xyws.h), 32 bytes: one completed recv."""
    _fields_ = [("conn", C.c_uint32), ("flags", C.c_uint32), ("off", C.c_uint64), ("len", C.c_uint64),
                ("at", C.c_uint64)]


class InboxCarry(C.Structure):
    """xyws_inbox_carry (include/xyws.h), 32 bytes; all zero: fresh, HTTP state."""
    _fields_ = [("http_len", C.c_uint64), ("bytes_total", C.c_uint64), ("state", C.c_uint32), ("status", C.c_uint32),
                ("reserved", C.c_uint64)]


class InboxConn(C.Structure):
    """xyws_inbox_conn (include/xyws.h), 64 bytes: entry i is connection i of the sweep's tables."""
    _fields_ = [("buf", C.c_void_p), ("cap", C.c_uint64), ("carry", C.c_void_p), ("conn", C.c_void_p),
                ("aconn", C.c_void_p), ("aresult", C.c_void_p), ("flags", C.c_uint32), ("reserved0", C.c_uint32),
                ("reserved", C.c_uint64)]


class InboxResult(C.Structure):
    """xyws_inbox_result (include/xyws.h), 32 bytes."""
    _fields_ = [("len", C.c_uint64), ("lead", C.c_uint64), ("n_entries", C.c_uint32), ("status", C.c_uint32),
                ("reserved", C.c_uint64)]


class InboxSummary(C.Structure):
    """xyws_inbox_summary (include/xyws.h), 64 bytes."""
    _fields_ = [("n_entries", C.c_uint64), ("bytes", C.c_uint64), ("n_conns", C.c_uint32), ("n_opened", C.c_uint32),
                ("n_eof", C.c_uint32), ("n_broken", C.c_uint32), ("n_bad_entries", C.c_uint32), ("status", C.c_uint32),
                ("reserved", C.c_uint64 * 3)]


assert (C.sizeof(InboxHead), C.sizeof(InboxEntry), C.sizeof(InboxCarry), C.sizeof(InboxConn), C.sizeof(InboxResult),
        C.sizeof(InboxSummary)) == (32, 32, 32, 64, 32, 64)
IBE_EOF = 0x1  # xyws_inbox_entry.flags
IBC_NO_HANDSHAKE = 0x1  # xyws_inbox_conn.flags
IB_HTTP, IB_OPEN, IB_DEAD = 0, 1, 2  # xyws_inbox_carry.state
(IBR_EOF, IBR_DROPPED, IBR_REFUSED, IBR_BAD_TILING, IBR_OVERFLOW, IBR_BAD_RANGE, IBR_BAD_CONSUMED,
 IBR_OPENED) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80  # xyws_inbox_result.status
IBM_BAD_ENTRIES, IBM_BROKEN, IBM_CLIPPED = 0x1, 0x2, 0x4  # xyws_inbox_summary.status


class Table:
    """n rows of the ctypes structure `struct` (one of the row types above),
    filled by field name (`t[k].out_cap = ...`) and uploaded as they are: over
    `host`, the pinned tensor of a ring whose storage the rows then are, or
    freshly allocated and zero. The structures are the only statement of a
    row's layout in Python."""

    def __init__(self, struct, n, host=None):
        self.n, self.nbytes, self.host = n, C.sizeof(struct) * n, host
        rows = struct * max(n, 1)
        self.rows = rows() if host is None else rows.from_address(host.data_ptr())

    def __getitem__(self, k):
        return self.rows[k]

    def upload(self, to):
        """The table on the device. to: for a ring table its device tensor,
        whose first n rows are overwritten from the pinned rows without
        waiting; otherwise a device, where a new uint8 tensor of max(n, 1)
        rows is made."""
        import torch
        if self.host is not None:
            w = self.nbytes // self.host.element_size()
            to[:w].copy_(self.host[:w], non_blocking=True)
            return to
        import numpy as np
        return torch.from_numpy(np.frombuffer(self.rows, np.uint8)).to(to)


def read_rows(struct, t, n, first=0):
    """Host copies of rows first .. first + n - 1 of the device uint8 tensor t,
    which holds rows of the ctypes structure `struct` (synchronizes)."""
    size = C.sizeof(struct)
    raw = t[size * first:size * (first + n)].cpu().numpy().tobytes() if n else b""
    return [struct.from_buffer_copy(raw, size * k) for k in range(n)]


def alloc_rows(struct, n, device, zero=True, per=1):
    """A uint8 tensor for max(n, 1) * per rows of the ctypes structure `struct`
    on `device` (per: rows per connection), zeroed or left as allocated."""
    import torch
    make = torch.zeros if zero else torch.empty
    return make(max(n, 1) * per * C.sizeof(struct), dtype=torch.uint8, device=device)


def row_ptr(t, struct, k=0):
    """The address of row k of the uint8 tensor t, which holds rows of `struct`."""
    return t.data_ptr() + C.sizeof(struct) * k


_lib = None
_tools = None


def declared_symbols(header=HEADER):
    """Function names declared in include/xyws.h."""
    src = open(header).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char\*|uint64_t|void\s*\*|void)\s*(xyws_\w+)\s*\(",
                                 src, re.M)))


def lib_path(name="libxyws.so"):
    return os.path.join(PKG, name)


def load():
    """Load libxyws.so (raises if it was not built: no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # XYWS_LIB: an alternative in-tree build of the same library (A/B timing
    # of compile-time variants; scripts/exp_variants.sh)
    path = os.environ.get("XYWS_LIB") or lib_path()
    if not os.path.exists(path):
        raise XywsError(-2, f"{path} missing: build it with `python -m xynet_amd.build`")
    L = C.CDLL(path)
    u64, u32, u8, vp, i32 = C.c_uint64, C.c_uint32, C.c_uint8, C.c_void_p, C.c_int
    L.xyws_abi_version.restype = i32
    L.xyws_strerror.restype = C.c_char_p
    L.xyws_strerror.argtypes = [i32]
    L.xyws_ctx_create.restype = i32
    L.xyws_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.xyws_ctx_destroy.restype = i32
    L.xyws_ctx_destroy.argtypes = [vp]
    L.xyws_ctx_reserve.restype = i32
    L.xyws_ctx_reserve.argtypes = [vp, u64, u64]
    L.xyws_ctx_reserve_iov.restype = i32
    L.xyws_ctx_reserve_iov.argtypes = [vp, u64]
    L.xyws_ctx_last_device_error.restype = i32
    L.xyws_ctx_last_device_error.argtypes = [vp, C.POINTER(u32)]
    L.xyws_unmask.restype = i32
    L.xyws_unmask.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), vp]
    L.xyws_mask_bytes.restype = i32
    L.xyws_mask_bytes.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), vp]
    L.xyws_decode_indexed.restype = i32
    L.xyws_decode_indexed.argtypes = [vp, vp, u64, vp, u64, vp, u32, vp]
    L.xyws_debug_stats.restype = i32
    L.xyws_debug_stats.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    L.xyws_debug_policy.restype = i32
    L.xyws_debug_policy.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    L.xyws_debug_lattice.restype = i32
    L.xyws_debug_lattice.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    L.xyws_debug_records.restype = C.c_int64
    L.xyws_debug_records.argtypes = [vp, vp, C.POINTER(C.c_uint64), u64]
    # (no HIP call: the decode's host-side plan, tests/test_plan.py)
    L.xyws_debug_plan.restype = i32
    L.xyws_debug_plan.argtypes = [i32, C.POINTER(u64), u64, u64, u64, u32, C.POINTER(u64)]
    L.xyws_debug_plan_reserve.restype = i32
    L.xyws_debug_plan_reserve.argtypes = [i32, u64, u64, C.POINTER(u64)]
    L.xyws_decode_stream.restype = i32
    L.xyws_decode_stream.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u32, vp]
    L.xyws_decode_stream_iov.restype = i32
    L.xyws_decode_stream_iov.argtypes = [vp, vp, u32, vp, vp, vp, u64, vp, u32, vp]
    L.xyws_decode_streams.restype = i32
    L.xyws_decode_streams.argtypes = [vp, vp, u64, vp, u32, vp]
    # (no HIP call: window bytes, lanes per connection, connections per workgroup, grid cap)
    L.xyws_debug_streams_geometry.restype = i32
    L.xyws_debug_streams_geometry.argtypes = [C.POINTER(u64)]
    L.xyws_reply_streams.restype = i32
    L.xyws_reply_streams.argtypes = [vp, vp, vp, vp, u64, u64, u32, u8, u32, u32, vp, vp]
    # (no HIP call: frames per tile, bytes per copy step, grid cap, wave size)
    L.xyws_debug_reply_geometry.restype = i32
    L.xyws_debug_reply_geometry.argtypes = [C.POINTER(u64)]
    L.xyws_reassemble_streams.restype = i32
    L.xyws_reassemble_streams.argtypes = [vp, vp, vp, vp, u64, u32, vp, vp]
    # (no HIP call: frames per tile, bytes per copy step, grid cap, wave size)
    L.xyws_debug_reasm_streams_geometry.restype = i32
    L.xyws_debug_reasm_streams_geometry.argtypes = [C.POINTER(u64)]
    L.xyws_broadcast_streams.restype = i32
    L.xyws_broadcast_streams.argtypes = [vp, vp, vp, vp, u64, vp, vp, u64, u8, u32, vp, vp]
    # (no HIP call: members per tile of the wire build, bytes per fan-out step, grid cap, wave size)
    L.xyws_debug_broadcast_geometry.restype = i32
    L.xyws_debug_broadcast_geometry.argtypes = [C.POINTER(u64)]
    L.xyws_hold_streams.restype = i32
    L.xyws_hold_streams.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp]
    # (no HIP call: lanes per connection, bytes per line, bytes per copy step, grid cap)
    L.xyws_debug_hold_geometry.restype = i32
    L.xyws_debug_hold_geometry.argtypes = [C.POINTER(u64)]
    L.xyws_backlog_streams.restype = i32
    L.xyws_backlog_streams.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp]
    # (no HIP call: members per tile of the fold, bytes per delivery step, grid cap, wave size)
    L.xyws_debug_backlog_geometry.restype = i32
    L.xyws_debug_backlog_geometry.argtypes = [C.POINTER(u64)]
    L.xyws_roster_streams.restype = i32
    L.xyws_roster_streams.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(RosterText), u8, vp, vp, vp, vp]
    # (no HIP call: members per tile of the room pass, words per step of the joiner scan, bytes per delivery step, grid cap)
    L.xyws_debug_roster_geometry.restype = i32
    L.xyws_debug_roster_geometry.argtypes = [C.POINTER(u64)]
    L.xyws_accept_streams.restype = i32
    L.xyws_accept_streams.argtypes = [vp, vp, u64, u32, u32, vp, vp]
    # (host only: no context, no HIP call)
    L.xyws_accept_request.restype = i32
    L.xyws_accept_request.argtypes = [vp, u64, u32, u32, vp, u64, C.POINTER(AcceptResult)]
    # (no HIP call: lanes per connection, LDS bytes per wave at the largest max_request, lines staged per step, grid cap)
    L.xyws_debug_accept_geometry.restype = i32
    L.xyws_debug_accept_geometry.argtypes = [C.POINTER(u64)]
    # (no HIP call: xyws_accept_request over a host slab of n requests, on the calling thread)
    L.xyws_debug_accept_host.restype = i32
    L.xyws_debug_accept_host.argtypes = [vp, u64, u64, u64, u32, u32, vp, u64, u64, vp]
    L.xyws_route_build.restype = i32
    L.xyws_route_build.argtypes = [C.POINTER(Route), u32, u32, vp, u64, C.POINTER(u64)]
    # (host only: no context, no HIP call)
    L.xyws_route_lookup.restype = i32
    L.xyws_route_lookup.argtypes = [vp, u64, vp, u64, C.POINTER(RouteResult)]
    L.xyws_route_streams.restype = i32
    L.xyws_route_streams.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, u64, u32, u32, vp, vp]
    # (no HIP call: lanes per connection, target bytes per lane, staged bytes per wave, grid cap)
    L.xyws_debug_route_geometry.restype = i32
    L.xyws_debug_route_geometry.argtypes = [C.POINTER(u64)]
    # (no HIP call: the slot at which the chain of a key in normal form begins among `slots`)
    L.xyws_debug_route_home.restype = u32
    L.xyws_debug_route_home.argtypes = [vp, u32, u32]
    # (no HIP call: xyws_route_lookup over the targets of a host slab of n requests, on the calling thread)
    L.xyws_debug_route_host.restype = i32
    L.xyws_debug_route_host.argtypes = [vp, u64, vp, u64, vp, u64, u32, vp]
    L.xyws_outbox_scratch_bytes.restype = u64
    L.xyws_outbox_scratch_bytes.argtypes = [u64]
    L.xyws_outbox_map.restype = i32
    L.xyws_outbox_map.argtypes = [vp, C.POINTER(vp)]
    L.xyws_outbox_streams.restype = i32
    L.xyws_outbox_streams.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, u64, vp]
    # (no HIP call: connections per tile of the plan pass, bytes per step of the pack pass, its largest grid x and y)
    L.xyws_debug_outbox_geometry.restype = i32
    L.xyws_debug_outbox_geometry.argtypes = [C.POINTER(u64)]
    # (measurements: one device-to-host copy per sender, issued from C by the calling thread)
    L.xyws_debug_outbox_host_fetch.restype = i32
    L.xyws_debug_outbox_host_fetch.argtypes = [vp, vp, u64, vp, u64, vp]
    L.xyws_inbox_scratch_bytes.restype = u64
    L.xyws_inbox_scratch_bytes.argtypes = [u64, u64]
    L.xyws_inbox_streams.restype = i32
    L.xyws_inbox_streams.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, vp, vp, u64, vp]
    # (no HIP call: connections per tile, bytes per step of the copy pass, its largest grid x and y, the entry pass's grid)
    L.xyws_debug_inbox_geometry.restype = i32
    L.xyws_debug_inbox_geometry.argtypes = [C.POINTER(u64)]
    # (measurements: one host-to-device copy per entry, issued from C by the calling thread)
    L.xyws_debug_inbox_host_scatter.restype = i32
    L.xyws_debug_inbox_host_scatter.argtypes = [vp, vp, vp, u64, vp, vp]
    # (no HIP call: k_unmask_range's tile bytes, threads per workgroup, workgroups per CU; a context's scratch slots)
    L.xyws_debug_unmask_geometry.restype = i32
    L.xyws_debug_unmask_geometry.argtypes = [C.POINTER(u64)]
    # ABI 2
    L.xyws_parser_create.restype = i32
    L.xyws_parser_create.argtypes = [vp, C.POINTER(vp)]
    L.xyws_parser_destroy.restype = i32
    L.xyws_parser_destroy.argtypes = [vp]
    L.xyws_parser_reset.restype = i32
    L.xyws_parser_reset.argtypes = [vp]
    L.xyws_parser_parse.restype = i32
    L.xyws_parser_parse.argtypes = [vp, vp, u64, C.POINTER(u64), vp]
    L.xyws_parser_result.restype = i32
    L.xyws_parser_result.argtypes = [vp, C.POINTER(u8), vp, C.POINTER(u64)]
    L.xyws_header_build.restype = u64
    L.xyws_header_build.argtypes = [u8, vp, u64, vp]
    L.xyws_encode_frames.restype = i32
    L.xyws_encode_frames.argtypes = [vp, vp, u64, vp, u64, vp, u8, u32, vp, vp, u32, vp, u64, vp, vp, vp]
    L.xyws_classify_frames.restype = i32
    L.xyws_classify_frames.argtypes = [vp, vp, u64, vp, u64, vp, u64, u32, vp, vp, vp]
    L.xyws_reassemble.restype = i32
    L.xyws_reassemble.argtypes = [vp, vp, u64, vp, u64, vp, u32, vp, u64, vp, u64, vp, vp]
    L.xyws_reassemble_stream.restype = i32
    L.xyws_reassemble_stream.argtypes = [vp, vp, u64, vp, u64, vp, u32, vp, vp, vp, u64, vp, u64, vp, vp]
    L.xyws_arena_create.restype = i32
    L.xyws_arena_create.argtypes = [vp, vp, u64, u64, i32, C.POINTER(vp)]
    L.xyws_arena_destroy.restype = i32
    L.xyws_arena_destroy.argtypes = [vp]
    L.xyws_arena_host.restype = vp
    L.xyws_arena_host.argtypes = [vp]
    L.xyws_arena_submit.restype = i32
    L.xyws_arena_submit.argtypes = [vp, u64, u64, u32, C.POINTER(u64)]
    L.xyws_arena_poll.restype = i32
    L.xyws_arena_poll.argtypes = [vp, u64, vp]
    L.xyws_arena_wait.restype = i32
    L.xyws_arena_wait.argtypes = [vp, u64, vp]
    L.xyws_notifier_create.restype = i32
    L.xyws_notifier_create.argtypes = [i32, C.POINTER(vp)]
    L.xyws_notifier_destroy.restype = i32
    L.xyws_notifier_destroy.argtypes = [vp]
    L.xyws_notifier_signal.restype = i32
    L.xyws_notifier_signal.argtypes = [vp, u64]
    L.xyws_notifier_completed.restype = u64
    L.xyws_notifier_completed.argtypes = [vp]
    L.xyws_notifier_enqueue.restype = i32
    L.xyws_notifier_enqueue.argtypes = [vp, u64, vp]
    L.xyws_shard_plan.restype = i32
    L.xyws_shard_plan.argtypes = [vp, u64, vp, u32, C.POINTER(u64)]
    L.xyws_shard_plan_frames.restype = i32
    L.xyws_shard_plan_frames.argtypes = [vp, u64, u64, u32, C.POINTER(u64)]
    _lib = L
    return L


def load_tools():
    global _tools
    if _tools is not None:
        return _tools
    path = lib_path("libxyws_tools.so")
    if not os.path.exists(path):
        raise XywsError(-2, f"{path} missing: build it with `python -m xynet_amd.build`")
    T = C.CDLL(path)
    u64, u8, vp, i32 = C.c_uint64, C.c_uint8, C.c_void_p, C.c_int
    T.xyws_tools_fill_uniform.restype = i32
    T.xyws_tools_fill_uniform.argtypes = [vp, u64, u64, u8, u64, vp]
    T.xyws_tools_mixed_table.restype = u64
    T.xyws_tools_mixed_table.argtypes = [u64, u64, vp, u64, C.POINTER(u64)]
    T.xyws_tools_fill_mixed.restype = i32
    T.xyws_tools_fill_mixed.argtypes = [vp, u64, vp, u64, u64, vp]
    T.xyws_tools_digest.restype = i32
    T.xyws_tools_digest.argtypes = [vp, u64, vp, vp, vp]
    _tools = T
    return T


def route_table(exact=None, prefix=None, slots=0):
    """The blob xyws_route_build makes of {key bytes: room} for exact and for
    XYWS_ROUTE_PREFIX routes (host bytes). Route indices count the exact routes
    first, each dict in its own order."""
    routes = [(bytes(k), int(r), 0) for k, r in (exact or {}).items()] + \
             [(bytes(k), int(r), ROUTE_PREFIX) for k, r in (prefix or {}).items()]
    return route_table_of(routes, slots)


def route_table_of(routes, slots=0):
    """xyws_route_build over (key bytes, room, flags) triples (host bytes)."""
    lib = load()
    rows = (Route * max(len(routes), 1))()
    keep = [C.create_string_buffer(k, max(len(k), 1)) for k, _, _ in routes]
    for row, buf, (k, room, flags) in zip(rows, keep, routes):
        row.key, row.key_len, row.room, row.flags = C.addressof(buf), len(k), room, flags
    need = C.c_uint64()
    rc = lib.xyws_route_build(rows, len(routes), slots, None, 0, C.byref(need))
    if rc != -4:
        raise XywsError(rc if rc else -1, "xyws_route_build")
    blob = C.create_string_buffer(need.value)
    check(lib.xyws_route_build(rows, len(routes), slots, blob, need.value, C.byref(need)), "xyws_route_build")
    return blob.raw


def check(rc, what=""):
    if rc != XYWS_OK:
        raise XywsError(rc, what)
    return rc
