"""xyws_unsent_streams and xyws_unsent_view_streams on the device. Expected
values: the model (tests/unsent_model.py); integer work, so every byte of the
send buffers (guard bytes between and around them included), every carry and
every result row is compared exactly, and the device error word reads 0."""
import ctypes as C
import itertools

import numpy as np
import pytest

import outbox_model as OM
import unsent_model as M
from test_gpu_outbox import Box, PAD, conn, ctx, payload, ws  # noqa: F401 (ctx and ws are fixtures)
from test_gpu_room import vp
from test_gpu_streams import GUARD, as_array, download, ptr, upload
from xynet_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

JUNK, SWEEP = 0x5A5A5A5A5A5A5A5A, 0x80000001
PEND, OUT = 1040, 1100        # pend_cap: one step of a wave and a line; the send range behind it
TAILS = (0, 1, 15, 16, 17, 1023, 1024, 1025, PEND, PEND + 1)
QUIET = 250                   # connections with nothing pending in front: the cases lie across a tile seam


def case(t, old, sp, dp, pend_cap=PEND):
    """A tail of t bytes whose source begins at 16-byte phase sp and whose destination at phase dp."""
    mis = (dp + t) % 16
    sent = (sp - mis + old) % 16
    return dict(pend_cap=pend_cap, old=old, last=sent + t, report=(sent, SWEEP), mis=mis)


def run(ctx, cases):
    """One xyws_unsent_streams call over `cases`, held to the model byte for byte."""
    n, image, conns = len(cases), bytearray([GUARD]) * 64, []
    for k, c in enumerate(cases):
        if c.get("mis") is None:
            conns.append(dict(out=None, pend_cap=0, out_cap=0, carry=None if c.get("no_carry") else dict(pend_len=0, last_len=0)))
            continue
        image += bytes([GUARD]) * ((c["mis"] - len(image) - c["pend_cap"]) % 16)   # (below 16: neighbours share lines)
        out = len(image) + c["pend_cap"]
        image += payload(k, c["pend_cap"] + OUT)
        conns.append(dict(out=out, pend_cap=c["pend_cap"], out_cap=OUT, carry=dict(pend_len=c["old"], last_len=c["last"])))
    image += bytes([GUARD]) * 64
    slab = upload(as_array(bytes(image)))
    carries = upload(as_array(b"".join(bytes(_lib.UnsentCarry(
        pend_len=c["carry"]["pend_len"], last_len=c["carry"]["last_len"], sweep=7, flags=7, reserved=JUNK)
        if c["carry"] else _lib.UnsentCarry()) for c in conns)))
    tab = _lib.Table(_lib.UnsentConn, n)
    for i, c in enumerate(conns):
        tab[i].out, tab[i].pend_cap = (ptr(slab) + c["out"] if c["out"] is not None else 0), c["pend_cap"]
        tab[i].carry, tab[i].reserved = (_lib.row_ptr(carries, _lib.UnsentCarry, i) if c["carry"] else 0), JUNK
    reports = {i: c["report"] for i, c in enumerate(cases) if c.get("report")}
    rep = _lib.Table(_lib.UnsentReport, n)
    for i in range(n):  # (a connection without a report of this sweep still has the row of an earlier one)
        rep[i].sent, rep[i].sweep = reports.get(i, (3, SWEEP - 1))
    head = _lib.Table(_lib.UnsentHead, 1)
    head[0].sweep, head[0].reserved = SWEEP, JUNK
    need = ctx.L.xyws_unsent_scratch_bytes(n)
    results = torch.full((32 * n + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    scratch = torch.full((need + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    tables = [tab.upload("cuda"), rep.upload("cuda"), head.upload("cuda")]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ctx.L.xyws_unsent_streams(ctx.h, vp(tables[0]), n, vp(tables[1]), vp(tables[2]), vp(results), vp(scratch), need, s) == 0
    torch.cuda.synchronize()
    want = M.unsent(image, conns, reports, SWEEP)
    got = download(slab).tobytes()
    assert got == bytes(image), ("send buffers, first byte", next(i for i in range(len(image)) if got[i] != image[i]))
    rows = _lib.read_rows(_lib.UnsentResult, results, n)
    assert [(r.pend_len, r.moved, r.status, r.reserved0, r.reserved) for r in rows] == \
        [(w["pend_len"], w["moved"], w["status"], 0, 0) for w in want]
    assert bool((results[32 * n:] == GUARD).all()) and bool((scratch[need:] == GUARD).all())
    for i, (c, r) in enumerate(zip(conns, _lib.read_rows(_lib.UnsentCarry, carries, n))):
        k = c["carry"] or dict(pend_len=0, last_len=0, sweep=0, flags=0)   # (a row no connection names stays zero)
        assert (r.pend_len, r.last_len, r.sweep, r.flags) == (k["pend_len"], k["last_len"], k["sweep"], k["flags"]), i
        assert r.reserved == (JUNK if c["carry"] else 0), i
    return want


@pytest.mark.parametrize("sp,dp", list(itertools.product((0, 1, 15), repeat=2)))
def test_every_tail_at_every_phase(ctx, sp, dp):
    """Each tail length with the old tail empty, short and full (the destination
    below, at and above the source start; both directions overlap), three of
    them neighbours at a time; then the connections that move nothing."""
    cases = [dict() for _ in range(QUIET)] + [case(t, old, sp, dp) for t in TAILS for old in (0, 5, PEND)]
    cases += [case(10, 0, sp, dp, pend_cap=0),                                  # no room in front: any short send overflows
              dict(case(20, 5, sp, dp), report=(3, SWEEP - 1)),                 # a stale report: it took everything
              dict(case(20, 5, sp, dp), report=None),
              dict(pend_cap=64, old=9, last=30, report=(37, SWEEP), mis=dp),    # sent > last_len
              dict(no_carry=True)]
    want = run(ctx, cases)[QUIET:]
    status = [w["status"] for w in want]
    assert status[-5:] == [M.OVERFLOW, 0, 0, M.BAD_REPORT, 0] and status[-8:-5] == [M.OVERFLOW] * 3
    assert all(w["pend_len"] == t for t, w in zip(TAILS[:-1], want[::3]))
    assert sum(w["moved"] > 0 for w in want) >= 2 * len(TAILS)


def test_the_view_under_the_outbox(ctx):
    """xyws_unsent_view_streams over an outbox table, then xyws_outbox_streams on the view: what the model says of
    connections whose ranges begin pend_len bytes earlier and whose rows say pend_len more."""
    conns = [conn(0, 60, bcast=dict(send_len=33)), conn(1, 40, reply=dict(reply_len=12, status=OM.RPL_CLOSED)),
             conn(2, 50, bcast=dict(send_len=51)), conn(3, 30, backlog=dict(send_len=0), bcast=dict(send_len=9)),
             conn(4, 0, null=True, bcast=dict(send_len=5)), conn(5, 20), conn(6, 20, bcast=dict(send_len=7))]
    pends = [7, 16, 5, 3, 9, 11, 4]
    box, n = Box(conns), len(conns)
    offs = iter(box.sends.offs)
    us = [dict(out=None if c["out"] is None else next(offs), pend_cap=16, out_cap=len(c["out"] or b""),
               carry=dict(pend_len=p, last_len=99)) for c, p in zip(conns, pends)]
    us[6]["carry"] = None
    carries = upload(as_array(b"".join(bytes(_lib.UnsentCarry(pend_len=p, last_len=99, sweep=2, flags=1, reserved=JUNK)) for p in pends)))
    tab = _lib.Table(_lib.UnsentConn, n)
    for i, u in enumerate(us):
        tab[i].out, tab[i].pend_cap = (ptr(box.sends.t) + u["out"] if u["out"] is not None else 0), 16
        tab[i].carry = _lib.row_ptr(carries, _lib.UnsentCarry, i) if u["carry"] else 0
    utab = tab.upload("cuda")
    view = torch.full((64 * n + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    vrows = torch.full((32 * n + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ctx.L.xyws_unsent_view_streams(ctx.h, vp(utab), vp(box.tab_t), n, vp(view), vp(vrows), s) == 0
    want = M.view(us, [OM.full_len(c) for c in conns])
    image = box.sends.image.tobytes()
    seen = [dict(c, out=None if o is None else image[o:o + cap], backlog=dict(send_len=send)) for c, (o, cap, send) in zip(conns, want)]
    box.conns, box.tab_t, box.tab_image = seen, view[:64 * n], None
    ts, ps = box.outputs(1024)
    assert box.launch(ctx, ps, 1024) == 0
    torch.cuda.synchronize()
    for name, t, w in zip(("pack", "entries", "summary"), ts, box.expected(1024, 1024)[:3]):
        assert download(t).tobytes() == w.tobytes(), name
    rows = _lib.read_rows(_lib.OutboxConn, view, n)
    assert [(r.out or 0, r.out_cap, r.backlog, r.reserved[0], r.reserved[1]) for r in rows] == [
        (0 if o is None else ptr(box.sends.t) + o, cap, ptr(vrows) + 32 * i, 0, 0) for i, (o, cap, _) in enumerate(want)]
    assert bool((view[64 * n:] == GUARD).all()) and bool((vrows[32 * n:] == GUARD).all())
    got = _lib.read_rows(_lib.UnsentCarry, carries, n)
    assert [(r.pend_len, r.last_len, r.reserved) for r in got[:6]] == [(u["carry"]["pend_len"], u["carry"]["last_len"], JUNK) for u in us[:6]]
    assert got[6].last_len == 99 and [u["carry"]["last_len"] for u in us[:4]] == [7 + 33, 16 + 12, 5 + 50, 3 + 0]


def test_two_sweeps_through_the_group(ws, ctx):
    """connection_group.unsent and outbox(unsent=): connection 0 takes everything, 1 takes half, 2 has no room for
    its tail, 3 is silent. Sweep 2 sends `tail | new bytes`, and a close survives the view. With unsent=None
    outbox() is the call it was."""
    from test_gpu_roster import masked
    n, caps = 4, [64, 64, 2, 64]
    grp = ws.connection_group(n, cap=4, ctx=ctx)
    bufs = [torch.full((c + 256,), GUARD, dtype=torch.uint8, device="cuda") for c in caps]
    sends = [b[c:] for b, c in zip(bufs, caps)]
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")

    def sweep(u, pieces):
        dec = grp.decode([(i, upload(as_array(p)) if p else empty) for i, p in enumerate(pieces)])
        rep = grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                        action_mask=1 << _lib.ACT_PING)
        return rep, grp.outbox(rep, unsent=u)

    rep, ob = sweep(grp.unsent([], 1, caps, bufs), [masked(b"ping one", 0x89), masked(b"a longer ping", 0x89), masked(b"third", 0x89), b""])
    first = {e.conn: ob.bytes(k) for k, e in enumerate(ob.entries())}
    assert sorted(first) == [0, 1, 2] and all(first[i] == sends[i][:len(first[i])].cpu().numpy().tobytes() for i in first)
    plain = grp.outbox(rep, unsent=None)   # (as it ever was: rows over the sweep's items, nothing in front)
    assert [(e.conn, e.flags, e.len) for e in plain.entries()] == [(e.conn, e.flags, e.len) for e in ob.entries()]
    assert plain.pack() == ob.pack() and "view" not in plain._tensors
    half = len(first[1]) // 2
    u = grp.unsent([(1, half), (2, 1)], 2, caps)
    assert [u.result(i).status for i in range(n)] == [0, M.KEPT, M.OVERFLOW, 0] and u.pending(1) == first[1][half:]
    rep, ob = sweep(u, [b"", masked(b"\x03\xe8", 0x88), b"", b""])
    news = sends[1][:rep.result(1).reply_len].cpu().numpy().tobytes()
    assert [(e.conn, e.flags) for e in ob.entries()] == [(1, _lib.OB_CLOSE)] and news
    assert ob.bytes(0) == first[1][half:] + news and grp.unsent_carry(1).last_len == len(ob.bytes(0))
    assert grp.outbox(rep, unsent=u, pack_cap=0).bytes(0) == ob.bytes(0)   # (deferred: read in place)
    u = grp.unsent([], 3, caps)                                            # everything was taken
    assert [u.result(i).pend_len for i in range(n)] == [0] * n and grp.outbox(None, unsent=u).entries() == []
