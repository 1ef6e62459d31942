"""xyws_outbox_streams in plain Python, from the rules of include/xyws.h.

A connection is a dict: out (the bytes of its send buffer, or None), out_cap
(default len(out)), and the rows the sweep wrote for it, each a dict or None:
backlog {send_len}, bcast {send_len} (a roster row as well), reply {reply_len,
status}, accept {status, resp_len}. Nothing here looks at the library."""

CLOSE, OVERFLOW, TRUNCATED, DEFERRED = 0x1, 0x2, 0x4, 0x8  # entry flags
S_DEFERRED, S_TRUNCATED = 0x1, 0x2                          # summary status
RPL_CLOSED, RPL_OVERFLOW = 0x2, 0x4
ACC_ACCEPTED, ACC_REJECTED = 0x1, 0x2


def align16(v):
    return (v + 15) & ~15


def out_cap_of(c):
    if c.get("out") is None:
        return 0
    return c.get("out_cap", len(c["out"]))


def full_len(c):
    """Rule 1."""
    if c.get("backlog") is not None:
        return c["backlog"]["send_len"]
    if c.get("bcast") is not None:
        return c["bcast"]["send_len"]
    if c.get("reply") is not None:
        return c["reply"]["reply_len"]
    a = c.get("accept")
    if a is not None and a["status"] & (ACC_ACCEPTED | ACC_REJECTED):
        return a["resp_len"]
    return 0


def flags_of(c):
    """Rule 2 (without DEFERRED, which depends on the pack)."""
    f = 0
    r, a = c.get("reply"), c.get("accept")
    if (r is not None and r["status"] & RPL_CLOSED) or (a is not None and a["status"] & ACC_REJECTED):
        f |= CLOSE
    if r is not None and r["status"] & RPL_OVERFLOW:
        f |= OVERFLOW
    if full_len(c) > out_cap_of(c):
        f |= TRUNCATED
    return f


def outbox(conns, pack_cap, pack=None):
    """(entries, summary, writes): entries are dicts conn, flags, off, len,
    full_len in list order; summary a dict of the eight fields; writes
    {offset: bytes} of every packed slot, the pad included. pack_cap None: a
    null pack."""
    cap = 0 if pack_cap is None else pack_cap & ~15
    entries, writes, off = [], {}, 0
    for i, c in enumerate(conns):
        full, ocap = full_len(c), out_cap_of(c)
        n, f = min(full, ocap), flags_of(c)
        if not n and not f:
            continue
        slot = align16(n)
        if n and off + slot > cap:
            f |= DEFERRED
        elif n:
            writes[off] = bytes(c["out"][:n]) + bytes(slot - n)
        entries.append(dict(conn=i, flags=f, off=off, len=n, full_len=full))
        off += slot
    packed = [e for e in entries if e["len"] and not e["flags"] & DEFERRED]
    n_def = sum(1 for e in entries if e["flags"] & DEFERRED)
    n_trunc = sum(1 for e in entries if e["flags"] & TRUNCATED)
    summary = dict(n_entries=len(entries), pack_len=off,
                   packed_len=max((e["off"] + align16(e["len"]) for e in packed), default=0),
                   send_bytes=sum(e["len"] for e in entries),
                   n_close=sum(1 for e in entries if e["flags"] & CLOSE), n_truncated=n_trunc, n_deferred=n_def,
                   status=(S_DEFERRED if n_def else 0) | (S_TRUNCATED if n_trunc else 0))
    return entries, summary, writes


def apply(writes, image):
    """The pack after the call: `image` (a bytearray) with the packed slots written."""
    for off, b in writes.items():
        image[off:off + len(b)] = b
    return image
