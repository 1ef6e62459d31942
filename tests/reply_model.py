"""Python model of xyws_reply_streams for ONE connection (include/xyws.h states
the semantics; the step numbers below are the header's). Verdicts come from
oracle.classify and headers from oracle.header_build, so the model adds only
the part that is new: the carried prefix, clipping at the batch end, the
close frame, the carry and the result."""
import numpy as np

NPOS = (1 << 64) - 1
TRUNCATED, CLOSED, OVERFLOW = 1, 2, 4
OP_MASK, OP_PING, OP_PONG, FIN, HAS_MASK = 0x0F, 0x09, 0x0A, 0x10, 0x20
ENC_FRAME_OPCODE = 1
ACT_DATA, ACT_PING, ACT_PONG, ACT_CLOSE = 0, 1, 2, 3
POL_FRAGMENTS, POL_UNMASKED, POL_STRICT, POL_REFERENCE = 1, 2, 4, 8
# the two modes the issue names: the reference's echo (close test included, every reply FIN|TEXT) and the RFC one
# (the frame's own opcode, a ping answered as a pong)
MODES = {"reference": dict(policy=POL_REFERENCE, flags=FIN | 1, enc_opts=0, action_mask=1 << ACT_DATA),
         "rfc": dict(policy=0, flags=0, enc_opts=ENC_FRAME_OPCODE, action_mask=(1 << ACT_DATA) | (1 << ACT_PING))}


class Carry:
    """xyws_reply_carry."""
    FIELDS = ("frame_remaining", "frames_seen", "replies_total", "close_code", "echoing", "status")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw.get(f, 0))

    def copy(self):
        return Carry(**{f: getattr(self, f) for f in self.FIELDS})

    def as_tuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def pack(self):
        return (self.frame_remaining.to_bytes(8, "little") + self.frames_seen.to_bytes(8, "little") +
                self.replies_total.to_bytes(8, "little") + self.close_code.to_bytes(2, "little") +
                bytes([self.echoing, self.status]) + bytes(4))


def result(reply_len=0, first_close=NPOS, answered=0, close_code=0, status=0):
    return dict(reply_len=reply_len, first_close=first_close, answered=answered, close_code=close_code, status=status)


def reply_flags(flags, enc_opts, fflags):
    if not enc_opts & ENC_FRAME_OPCODE:
        return flags
    op = fflags & OP_MASK
    return (OP_PONG if op == OP_PING else op) | (fflags & FIN) | (flags & HAS_MASK)


def close_frame(code):
    return bytes([0x88, 0x02, code >> 8, code & 0xFF])  # websocket_send_close


def reply(oracle, buf, frames, rc, out_cap, max_payload, policy, flags, enc_opts, action_mask, nframes=None,
          cap=None, frames_null=False):
    """One call for one connection. buf: the decoded bytes (uint8 array);
    frames: the table (oracle Frame list); nframes / cap / frames_null: what
    dev_nframes[i], xyws_conn.cap and a null xyws_conn.frames would say
    (default: the table as it is). rc: a Carry, or None for a null pointer.
    Returns (written, res, verdicts, carry): written = the first
    min(reply_len, out_cap) reply bytes; verdicts None when none are stored."""
    t = len(frames) if nframes is None else nframes
    cap = len(frames) if cap is None else cap
    keep = rc is not None
    rc = rc.copy() if keep else Carry()
    ln = int(buf.size)
    if rc.status & OVERFLOW or t > cap or (frames_null and t > 0):  # 1
        rc.status |= OVERFLOW
        return b"", result(close_code=rc.close_code, status=OVERFLOW), None, rc if keep else None
    if rc.close_code:  # 2
        return b"", result(close_code=rc.close_code, status=CLOSED), None, rc if keep else None
    out = bytearray()
    k = min(rc.frame_remaining, ln)  # 3
    if rc.echoing:
        out += buf[:k].tobytes()
    rc.frame_remaining -= k
    frames = list(frames)[:t]
    verdicts, first = oracle.classify(buf, frames, max_payload, policy)  # 4
    c = t if first == NPOS else first
    answered = 0
    for j in range(c):  # 5
        f = frames[j]
        ans = (action_mask >> verdicts[j].action) & 1
        off = f.payload_off & NPOS
        inb = min(f.payload_len, ln - off) if off < ln else 0
        if ans:
            out += oracle.header_build(reply_flags(flags, enc_opts, f.flags), None, f.payload_len)
            out += buf[off:off + inb].tobytes()
            answered += 1
        rc.frame_remaining, rc.echoing = f.payload_len - inb, ans
    status = 0
    if c < t:  # 6
        rc.close_code = verdicts[c].close_code
        out += close_frame(rc.close_code)
        status |= CLOSED
    rc.frames_seen += t  # 7
    rc.replies_total += answered
    if len(out) > out_cap:  # 8
        status |= TRUNCATED
    res = result(len(out), c if c < t else NPOS, answered, rc.close_code, status)
    return bytes(out[:out_cap]), res, verdicts, rc if keep else None


def as_array(b):
    return np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(0, np.uint8)


def run_split(oracle, wire, cuts, mode, max_payload=1 << 20, out_caps=None):
    """The stream `wire` cut at `cuts` (ascending byte positions), each piece
    decoded from the chained decode carry (oracle.decode_stream) and answered
    by the model. Returns a list of per-call tuples (decoded piece, frames,
    decode carry after, written, res, verdicts, reply carry after)."""
    calls, dc, rc, prev = [], None, Carry(), 0
    for i, cut in enumerate(list(cuts) + [len(wire)]):
        piece = as_array(wire[prev:cut])
        prev = cut
        fr, dc, n = oracle.decode_stream(piece, carry_in=dc)
        assert n == len(fr)
        cap = out_caps[i] if out_caps is not None else piece.size + 13
        w, res, vd, rc = reply(oracle, piece, fr, rc, cap, max_payload, **MODES[mode] if isinstance(mode, str) else mode)
        calls.append((piece, fr, dc, w, res, vd, rc))
    return calls


def unsplit(oracle, wire, mode, max_payload=1 << 20):
    """What the issue's main statement expects of the whole stream:
    oracle.encode_frames of the frames before the first close with the
    verdicts of oracle.classify, then the close frame if any."""
    m = MODES[mode] if isinstance(mode, str) else mode
    buf = as_array(wire)
    fr, _, n = oracle.decode_stream(buf)
    assert n == len(fr)
    verdicts, first = oracle.classify(buf, fr, max_payload, m["policy"])
    c = n if first == NPOS else first
    # (a frame cut by the stream's end: only its bytes present are echoed)
    head = [f for f in fr[:c]]
    out, _, total = oracle.encode_frames(buf, head, m["flags"], m["enc_opts"], None, verdicts[:c], m["action_mask"])
    out = bytearray(out)
    if c and (m["action_mask"] >> verdicts[c - 1].action) & 1:
        f = head[-1]
        missing = f.payload_off + f.payload_len - buf.size
        if missing > 0:
            del out[len(out) - missing:]  # (the oracle pads bytes past the source with zeros)
    if c < n:
        out += close_frame(verdicts[c].close_code)
    return bytes(out)
