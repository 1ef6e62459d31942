"""xyws_inbox_streams in plain Python, from the rules of include/xyws.h.

A connection is a dict: cap (the size of its receive range), carry (a dict
http_len, bytes_total, state, status; fresh() is the all-zero one), flags
(NO_HANDSHAKE or 0), aresult (None, or a dict status, consumed: the accept row
as the previous sweep left it), has_conn / has_aconn (whether it names a
xyws_conn / xyws_accept_conn row, default True). An entry is a dict conn,
flags, off, len, at. Nothing here looks at the library."""

EOF_E = 0x1                 # entry flags
NO_HANDSHAKE = 0x1          # iconn flags
HTTP, OPEN, DEAD = 0, 1, 2  # carry.state
(R_EOF, R_DROPPED, R_REFUSED, R_BAD_TILING, R_OVERFLOW, R_BAD_RANGE, R_BAD_CONSUMED,
 R_OPENED) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80  # result / carry status
STICKY = R_EOF | R_REFUSED | R_BAD_TILING | R_OVERFLOW | R_BAD_RANGE | R_BAD_CONSUMED
S_BAD_ENTRIES, S_BROKEN, S_CLIPPED = 0x1, 0x2, 0x4  # summary status
ACC_ACCEPTED, ACC_REJECTED = 0x1, 0x2
U64 = (1 << 64) - 1


def fresh():
    return dict(http_len=0, bytes_total=0, state=HTTP, status=0)


def inbox(conns, head_m, head_pack_len, entries, m_cap, pack_cap):
    """One sweep. Returns (results, summary, rows, carries, writes):
    results[i] = dict len, lead, n_entries, status; summary a dict of the eight
    fields; rows[i] = dict conn_off, conn_len, aconn_len (conn->buf is buf +
    conn_off, aconn->buf is buf); carries[i] the carry afterwards (the inputs
    are not changed); writes = [(conn, range offset, pack offset, len)] for
    every byte run placed."""
    n = len(conns)
    M = min(head_m, m_cap)                                   # rule 1
    P = min(head_pack_len, pack_cap)
    T, S, cnt, eof, bad_range = [0] * n, [0] * n, [0] * n, [False] * n, [False] * n
    valid = [[] for _ in range(n)]
    n_bad = 0
    for e in entries[:M]:
        c = e["conn"]
        if c >= n:
            n_bad += 1
            continue
        cnt[c] += 1
        eof[c] = eof[c] or bool(e["flags"] & EOF_E)
        if e["off"] <= P and e["len"] <= P - e["off"]:
            S[c] += e["len"]                                 # rule 2
            T[c] = max(T[c], min(e["at"] + e["len"], U64))
            valid[c].append(e)
        else:
            n_bad += 1
            bad_range[c] = True
    results, rows, carries, writes = [], [], [], []
    n_opened = n_broken = 0
    for i, c in enumerate(conns):
        cr = dict(c.get("carry") or fresh())
        st, sticky, now = cr["state"], cr["status"], 0
        http_len = cr["http_len"]
        A = kept = lead = placed = 0
        opened = broken = False
        if eof[i]:
            sticky |= R_EOF                                  # rule 6
        if st >= DEAD:                                       # rule 3
            st = DEAD
        elif st == HTTP:
            a = c.get("aresult")
            if c.get("flags", 0) & NO_HANDSHAKE:
                st, http_len = OPEN, 0
            elif a is not None and a["status"] & ACC_REJECTED:
                st = DEAD
                sticky |= R_REFUSED
            elif a is not None and a["status"] & ACC_ACCEPTED:
                if a["consumed"] > http_len:
                    broken = True
                    sticky |= R_BAD_CONSUMED
                else:
                    opened, st = True, OPEN
                    kept = http_len - a["consumed"]
                    lead = a["consumed"] if kept else 0
        if st == DEAD:
            if cnt[i]:
                now |= R_DROPPED
        else:                                                # rule 4
            if not broken:
                A = http_len if (st == HTTP or kept) else 0
            if bad_range[i]:
                sticky |= R_BAD_RANGE
                broken = True
            if S[i] != T[i]:
                sticky |= R_BAD_TILING
                broken = True
            if A + T[i] > c["cap"]:
                sticky |= R_OVERFLOW
                broken = True
            if broken:
                st, opened, kept, lead = DEAD, False, 0, 0
            else:
                placed = T[i]
                writes += [(i, A + e["at"], e["off"], e["len"]) for e in valid[i] if e["len"]]
        row = dict(conn_off=0, conn_len=0, aconn_len=0)      # rule 5
        if st == OPEN:
            row.update(conn_off=lead, conn_len=kept + T[i])
            http_len = 0
        elif st == HTTP:
            http_len += T[i]
            row.update(aconn_len=http_len if T[i] else 0)
        n_opened += opened
        n_broken += broken
        carries.append(dict(http_len=http_len, bytes_total=cr["bytes_total"] + placed, state=st, status=sticky))
        results.append(dict(len=placed, lead=lead, n_entries=cnt[i],
                            status=sticky | now | (R_OPENED if opened else 0)))   # rule 7
        rows.append(row)
    summary = dict(n_entries=M, bytes=sum(r["len"] for r in results), n_conns=sum(1 for k in cnt if k),
                   n_opened=n_opened, n_eof=sum(eof), n_broken=n_broken, n_bad_entries=n_bad,
                   status=(S_BAD_ENTRIES if n_bad else 0) | (S_BROKEN if n_broken else 0) |
                   (S_CLIPPED if head_m > m_cap else 0))
    return results, summary, rows, carries, writes


def apply(writes, pack, ranges):
    """The receive ranges after the sweep: ranges[i] (a bytearray) with
    connection i's byte runs written, in list order."""
    for i, dst, off, n in writes:
        ranges[i][dst:dst + n] = pack[off:off + n]
    return ranges


def cut(total, pieces, rng):
    """`total` bytes cut into `pieces` runs (some may be empty) at seeded points: the run lengths."""
    points = sorted(rng.randint(0, total) for _ in range(pieces - 1)) if pieces > 0 else []
    edges = [0] + points + [total]
    return [b - a for a, b in zip(edges, edges[1:])] if pieces > 0 else []
