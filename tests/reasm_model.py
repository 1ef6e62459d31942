"""Plain-Python model of xyws_reassemble_stream (include/xyws.h): one call's
expected output bytes, records and carry, bit for bit. A sequential walk of
the batch (no scans, no tiles), written from the header's text, so that the
device path and this model are two formulations of the same rules. The model
itself is held to the unsplit stream's xyws_reassemble by
tests/test_reasm_model.py."""
import struct

NPOS = (1 << 64) - 1
REASM_UTF8 = 0x1
COMPLETE, UTF8_BAD, INTERRUPTED, TRUNCATED, ORPHANS, CONTINUED, UNCHECKED = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
OP_TEXT, OP_BINARY = 1, 2
STICKY = UTF8_BAD | UNCHECKED


class Carry:
    """xyws_msg_carry as a host object (pack() = its 64 bytes)."""
    FIELDS = ("length", "nframes", "first_frame", "frame_remaining", "frames_seen", "status", "opcode",
              "frame_member", "utf8")

    def __init__(self, **kw):
        self.length = self.nframes = self.first_frame = self.frame_remaining = self.frames_seen = 0
        self.status = self.opcode = self.frame_member = 0
        self.utf8 = b""
        for k, v in kw.items():
            setattr(self, k, v)

    def pack(self):
        return struct.pack("<5QIBBB3s14s", self.length, self.nframes, self.first_frame, self.frame_remaining,
                           self.frames_seen, self.status, self.opcode, self.frame_member, len(self.utf8),
                           self.utf8.ljust(3, b"\0"), b"")

    @classmethod
    def unpack(cls, raw):
        v = struct.unpack("<5QIBBB3s14s", bytes(raw))
        return cls(length=v[0], nframes=v[1], first_frame=v[2], frame_remaining=v[3], frames_seen=v[4],
                   status=v[5], opcode=v[6], frame_member=v[7], utf8=v[9][:v[8]])

    def as_tuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def __eq__(self, o):
        return self.as_tuple() == o.as_tuple()

    def __repr__(self):
        return "Carry(" + ", ".join(f"{f}={getattr(self, f)!r}" for f in self.FIELDS) + ")"


def lead_len(c):
    return 4 if c >= 0xF0 else 3 if c >= 0xE0 else 2 if c >= 0xC0 else 0


def _seq_bad(seq):
    """A whole sequence (lead + lead_len - 1 bytes): its continuation bytes and
    the second-byte rules."""
    c = seq[0]
    if any((b & 0xC0) != 0x80 for b in seq[1:]):
        return True
    c1 = seq[1]
    return (c == 0xE0 and c1 < 0xA0) or (c == 0xED and c1 > 0x9F) or (c == 0xF0 and c1 < 0x90) or \
        (c == 0xF4 and c1 > 0x8F)


def utf8_bad(prefix, data, length, complete):
    """xyws_reassemble's per-byte rules over `data` (the bytes of a message
    that lie in the output, of `length` delivered), `prefix` being the carried
    tail (the bytes before data[0] in the message). complete: the message is
    COMPLETE and not TRUNCATED (a sequence cut by its end is then invalid)."""
    n = len(data)
    for q in range(n):
        ch = data[q]
        if ch < 0x80:
            continue
        if ch < 0xC0:
            claimed = False
            for d in (1, 2, 3):
                p = q - d
                if p < -len(prefix):
                    break
                pb = data[p] if p >= 0 else prefix[len(prefix) + p]
                if lead_len(pb) > d:
                    claimed = True
                    break
            if not claimed:
                return True
        elif ch in (0xC0, 0xC1) or ch >= 0xF5:
            return True
        else:
            ln = lead_len(ch)
            if q + ln > length or q + ln > n:
                if complete:
                    return True
            elif _seq_bad(data[q:q + ln]):
                return True
    if prefix:
        need = lead_len(prefix[0]) - len(prefix)
        if need > 0:
            if n >= need:
                if _seq_bad(prefix + data[:need]):
                    return True
            elif complete:
                return True
    return False


def cut_tail(seq):
    """The bytes from the earliest lead in the last 3 bytes whose sequence runs
    past the end."""
    s3 = seq[-3:]
    for d in range(len(s3), 0, -1):
        if lead_len(s3[-d]) > d:
            return bytes(s3[-d:])
    return b""


def feed(src, frames, opts, carry=None, out_cap=None, msg_cap=None):
    """One xyws_reassemble_stream call. src: the decoded batch; frames: its
    descriptors (objects with payload_off, payload_len, flags); carry: Carry or
    None (fresh). Returns (out bytes written, records, carry out, nmsgs):
    records = the stored ones, tuples (first_frame, nframes, out_off, length,
    status, opcode)."""
    mc = carry if carry is not None else Carry()
    L = len(src)
    n = len(frames)
    if out_cap is None:
        out_cap = L
    if msg_cap is None:
        msg_cap = n + 1
    utf8 = bool(opts & REASM_UTF8) and out_cap > 0 and msg_cap > 0
    out = bytearray()
    recs = []  # dicts, in order of their start
    cur = None
    pending = False
    if mc.opcode:
        cur = dict(first=NPOS, nframes=0, off=0, length=0, status=CONTINUED | (mc.status & STICKY),
                   op=mc.opcode, fin=bool(mc.status & COMPLETE), cont=True)
        recs.append(cur)
    else:
        pending = bool(mc.status & ORPHANS)
    h = min(mc.frame_remaining, L)
    rem = mc.frame_remaining - h
    member = mc.frame_member if rem else 0
    if cur is not None and mc.frame_member:
        out += src[:h]
        cur["length"] += h
    if cur is not None and cur["fin"] and rem == 0:
        cur["status"] |= COMPLETE
        cur = None
    for i, f in enumerate(frames):
        op, fin = f.flags & 0x0F, bool(f.flags & 0x10)
        poff = f.payload_off
        avail = min(f.payload_len, L - poff) if 0 <= poff < L else 0
        frem = f.payload_len - avail
        joined = False
        if op in (OP_TEXT, OP_BINARY):
            if cur is not None:
                cur["status"] |= INTERRUPTED
            cur = dict(first=i, nframes=0, off=len(out), length=0, status=ORPHANS if pending else 0, op=op,
                       fin=False, cont=False)
            pending = False
            recs.append(cur)
            joined = True
        elif op == 0:
            if cur is not None and not cur["fin"]:
                joined = True
            else:
                pending = True
        if joined:
            out += src[poff:poff + avail]
            cur["length"] += avail
            cur["nframes"] += 1
            if fin:
                cur["fin"] = True
                if frem == 0:
                    cur["status"] |= COMPLETE
                    cur = None
        rem = frem
        member = 1 if (frem and joined) else 0
    # per call: truncation, validation
    for k, r in enumerate(recs):
        if r["off"] + r["length"] > out_cap:
            r["status"] |= TRUNCATED
    for k, r in enumerate(recs[:msg_cap]):
        if not utf8 or r["op"] != OP_TEXT or (r["status"] & (UTF8_BAD | UNCHECKED)):
            continue
        data = bytes(out[r["off"]:min(r["off"] + r["length"], out_cap)])
        prefix = mc.utf8 if r["cont"] else b""
        complete = bool(r["status"] & COMPLETE) and not (r["status"] & TRUNCATED)
        if utf8_bad(prefix, data, r["length"], complete):
            r["status"] |= UTF8_BAD
    co = Carry(frame_remaining=rem, frames_seen=mc.frames_seen + n)
    if cur is not None:
        k = len(recs) - 1
        stored = k < msg_cap
        co.opcode = cur["op"]
        co.frame_member = member
        co.length = (mc.length if cur["cont"] else 0) + cur["length"]
        co.nframes = (mc.nframes if cur["cont"] else 0) + cur["nframes"]
        co.first_frame = mc.first_frame if cur["cont"] else mc.frames_seen + cur["first"]
        st = COMPLETE if cur["fin"] else 0
        bad = bool(cur["status"] & UTF8_BAD) if stored else bool(cur["cont"] and mc.status & UTF8_BAD)
        unchecked = cur["op"] == OP_TEXT and (bool(cur["cont"] and mc.status & UNCHECKED) or not utf8 or
                                             bool(cur["status"] & TRUNCATED) or not stored)
        if bad:
            st |= UTF8_BAD
        if unchecked:
            st |= UNCHECKED
        co.status = st
        if cur["op"] == OP_TEXT and not bad and not unchecked:
            seq = (mc.utf8 if cur["cont"] else b"") + bytes(out[cur["off"]:cur["off"] + cur["length"]])
            co.utf8 = cut_tail(seq)
    else:
        co.frame_member = 0
        co.status = ORPHANS if pending else 0
    records = [(r["first"], r["nframes"], r["off"], r["length"], r["status"], r["op"]) for r in recs[:msg_cap]]
    return bytes(out[:out_cap]), records, co, len(recs)


def fold(folded, records, frames_seen):
    """Merge one call's records into the stream's list (lists of 6 fields,
    TRUNCATED dropped): a CONTINUED record adds to the message before it."""
    for (first, nfr, off, length, status, op) in records:
        status &= ~TRUNCATED
        if status & CONTINUED:
            m = folded[-1]
            assert m[5] == op
            m[1] += nfr
            m[3] += length
            m[4] |= status & ~CONTINUED
        else:
            folded.append([first + frames_seen, nfr, None, length, status, op])
    return folded
