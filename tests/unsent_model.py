"""Plain-Python model of xyws_unsent_streams and xyws_unsent_view_streams
(include/xyws.h) over one bytearray that holds every connection's send buffer.
A connection: dict(out=offset of its send range in the image, or None,
pend_cap=..., out_cap=..., carry=dict(pend_len, last_len, sweep, flags) or None)."""
KEPT, OVERFLOW, BAD_REPORT = 0x1, 0x2, 0x4


def unsent(image, conns, reports, sweep):
    """Sweep start. reports: {i: (sent, stamp)}. Moves the tails inside `image`,
    rewrites the carries; returns the result rows."""
    results = []
    for i, c in enumerate(conns):
        carry = c["carry"]
        if carry is None:
            results.append(dict(pend_len=0, moved=0, status=0))
            continue
        last, status, moved, pend = carry["last_len"], 0, 0, 0
        sent, stamp = reports.get(i, (last, sweep))
        if stamp != sweep:
            sent = last
        if sent > last:
            sent, status = last, BAD_REPORT
        t = last - sent
        if t and c["out"] is not None and t <= c["pend_cap"]:
            src = c["out"] - min(carry["pend_len"], c["pend_cap"]) + sent
            dst = c["out"] - t
            pend, status = t, status | KEPT
            if src != dst:
                image[dst:dst + t] = bytes(image[src:src + t])
                moved = t
        elif t:
            status |= OVERFLOW
        carry.update(pend_len=pend, last_len=pend, sweep=sweep, flags=status)
        results.append(dict(pend_len=pend, moved=moved, status=status))
    return results


def view(conns, full_lens):
    """Sweep end. full_lens[i]: rule 1 of xyws_outbox_streams for connection i.
    Sets every carry's last_len; returns per connection (out', out_cap', send_len)."""
    rows = []
    for c, full in zip(conns, full_lens):
        carry, out = c["carry"], c["out"]
        cap = c["out_cap"] if out is not None else 0
        pend = carry["pend_len"] if carry is not None and out is not None else 0
        if carry is not None:
            carry["last_len"] = pend + min(full, cap)
        rows.append((None if out is None else out - pend, cap + pend if out is not None else cap, pend + full))
    return rows
