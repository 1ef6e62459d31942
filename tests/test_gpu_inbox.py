"""xyws_inbox_streams on the device, through the C-ABI: a sweep's pack and entry
list scattered into the connections' receive ranges, with the carries and the
buf and len words of the resident xyws_conn and xyws_accept_conn rows. Expected
values: the model (tests/inbox_model.py), which tests/test_inbox_model.py holds
to hand-computed answers. Bar: bit-exact. One device image holds the receive
ranges, the row tables, the carries, the result table and the summary, with
guard bytes (0xA5) around and between them and junk in every field the call has
no business with; after every call the whole image equals the model's. The
iconn table, the head, the entries and the pack are unchanged; the device error
word reads 0.

Tile, copy step and grid sizes come from xyws_debug_inbox_geometry."""
import ctypes as C
import random

import numpy as np
import pytest

import inbox_model as M
from test_gpu_streams import GUARD, as_array, download, ptr, upload
from xynet_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
JUNK = 0x5A5A5A5A5A5A5A5A  # in every field of a row that the call has no business with
JUNK32 = 0x5A5A5A5A
PAD = 64                   # guard bytes between the regions of the image
ENT = np.dtype([("conn", "<u4"), ("flags", "<u4"), ("off", "<u8"), ("len", "<u8"), ("at", "<u8")])
POISON = dict(conn=0, flags=M.EOF_E, off=0, len=1, at=0)  # behind the entries of a list: it shows if it is read


@pytest.fixture(scope="module")
def ws():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xynet_amd import websocket
    return websocket


@pytest.fixture()
def ctx(ws):
    """A context of the test's own; the device error word must read 0 at the end."""
    c = ws.Context(0)
    yield c
    assert c.last_device_error() == 0
    c.close()


def geometry():
    out = (C.c_uint64 * 5)()
    assert _lib.load().xyws_debug_inbox_geometry(out) == 0
    return list(out)


def vp(t):
    return C.c_void_p(ptr(t))


def payload(k, n):
    """n nonzero bytes that are not the guard and differ from entry to entry."""
    v = (np.arange(n, dtype=np.uint32) * 7 + 13 * k + 1) % 251 + 1
    v[v == GUARD] = 3
    return v.astype(np.uint8).tobytes()


def ent(c, off, n, at, flags=0):
    return dict(conn=c, off=off, len=n, at=at, flags=flags)


def conn(cap, carry=None, flags=0, aresult=None, mis=None, null_rows=False):
    return dict(cap=cap, carry=carry, flags=flags, aresult=aresult, mis=mis, null_rows=null_rows)


def entries_image(entries, room):
    a = np.zeros(max(room, 1), ENT)
    for f in ENT.names:
        a[f][:len(entries)] = [e[f] for e in entries]
    return a.view(np.uint8).reshape(-1)


def mapped(t):
    d = C.c_void_p()
    if _lib.load().xyws_outbox_map(C.c_void_p(t.data_ptr()), C.byref(d)) != 0:
        pytest.skip("xyws_outbox_map refuses torch's pinned memory: it is not mapped for the device")
    return d.value


class Pack:
    """A sweep's pack built entry by entry: add() returns the offset of the bytes it appends."""

    def __init__(self):
        self.b = bytearray()

    def add(self, data, residue=None):
        if residue is not None:
            self.b += bytes([0xEE]) * ((residue - len(self.b)) % 16)
        off = len(self.b)
        self.b += data
        return off


class World:
    """The state of n connections on the device in one guarded image, and one
    xyws_inbox_streams call after another over it, each held to the model."""

    def __init__(self, conns, apart=False):
        self.conns, self.n = conns, len(conns)
        n, p, self.offs = self.n, PAD, []
        for i, c in enumerate(conns):
            if apart or c["mis"] is not None:
                p = ((p + 31) & ~15) + (i % 16 if c["mis"] is None else c["mis"])
            self.offs.append(p)
            p += c["cap"]
        self.tab = {}
        for name, size in (("conns", 64 * n), ("aconns", 32 * n), ("aresults", 32 * n), ("carries", 32 * n),
                           ("results", 32 * n), ("summary", 64)):
            p = (p + PAD + 63) & ~63
            self.tab[name] = p
            p += size
        self.image = np.full(p + PAD, GUARD, np.uint8)
        self.words("conns", 8)[:] = JUNK
        self.words("aconns", 4)[:] = JUNK
        ar, ca = self.words("aresults", 4), self.words("carries", 4)
        ar[:] = JUNK
        for i, c in enumerate(conns):
            a = c["aresult"] or dict(status=0, consumed=0)
            ar[i, 0] = a["status"] | (JUNK32 << 32)
            ar[i, 1] = a["consumed"] | (JUNK32 << 32)
            cr = c["carry"] or M.fresh()
            ca[i] = [cr["http_len"], cr["bytes_total"], cr["state"] | (cr["status"] << 32), JUNK]
        self.t = upload(self.image)
        self.base = ptr(self.t)
        assert self.base % 64 == 0
        tab = np.zeros((max(n, 1), 8), np.uint64)
        for i, c in enumerate(conns):
            rows = [0, 0, 0] if c["null_rows"] else [self.base + self.tab["conns"] + 64 * i,
                                                      self.base + self.tab["aconns"] + 32 * i,
                                                      self.base + self.tab["aresults"] + 32 * i]
            tab[i] = [self.base + self.offs[i], c["cap"], self.base + self.tab["carries"] + 32 * i] + rows + \
                     [c["flags"] | (JUNK32 << 32), JUNK]
        self.iconn_image = tab.reshape(-1).view(np.uint8)
        self.iconn_t = upload(self.iconn_image)
        self.pending = []

    def words(self, name, per):
        o = self.tab[name]
        return self.image[o:o + 8 * per * self.n].view(np.uint64).reshape(self.n, per)

    def set_aresult(self, i, status, consumed):
        """The accept row of connection i as a sweep's xyws_accept_streams would leave it."""
        self.conns[i]["aresult"] = dict(status=status, consumed=consumed)
        ar = self.words("aresults", 4)
        ar[i, 0], ar[i, 1] = status | (JUNK32 << 32), consumed | (JUNK32 << 32)
        o = self.tab["aresults"] + 32 * i
        self.t[o:o + 32].copy_(upload(self.image[o:o + 32]))

    def range_bytes(self, i, n=None):
        return self.image[self.offs[i]:self.offs[i] + (self.conns[i]["cap"] if n is None else n)].tobytes()

    def inputs(self, entries, pack, m_cap, head_m, pack_len, pack_mis, pinned):
        """(tensors, pointers, images) of head, entries (m_cap + 1 rows, poison behind the list) and pack."""
        full = list(entries) + [POISON] * (m_cap + 1 - len(entries))
        head = np.array([head_m, pack_len, JUNK, JUNK], np.uint64).view(np.uint8)
        imgs = [np.concatenate([head, np.full(PAD, GUARD, np.uint8)]), entries_image(full, m_cap + 1),
                as_array(bytes([GUARD]) * (PAD + pack_mis) + bytes(pack) + bytes([GUARD]) * PAD)]
        if pinned:
            ts = [torch.from_numpy(a.copy()).pin_memory() for a in imgs]
            ps = [mapped(t) for t in ts]
        else:
            ts = [upload(a) for a in imgs]
            ps = [ptr(t) for t in ts]
        ps[2] += PAD + pack_mis
        return ts, ps, imgs, full

    def expect(self, full, pack, m_cap, head_m, pack_len, pack_cap, results=True):
        """The model's sweep applied to the image and to the model connections' carries."""
        res, summ, rows, cars, writes = M.inbox(self.conns, head_m, pack_len, full, m_cap, pack_cap)
        for i, dst, off, ln in writes:
            self.image[self.offs[i] + dst:self.offs[i] + dst + ln] = as_array(bytes(pack[off:off + ln]))
        cw, aw, ca = self.words("conns", 8), self.words("aconns", 4), self.words("carries", 4)
        rw = self.words("results", 4)
        for i, c in enumerate(self.conns):
            buf = self.base + self.offs[i]
            if not c["null_rows"]:
                cw[i, :2] = [buf + rows[i]["conn_off"], rows[i]["conn_len"]]
                aw[i, :2] = [buf, rows[i]["aconn_len"]]
            k = cars[i]
            ca[i, :3] = [k["http_len"], k["bytes_total"], k["state"] | (k["status"] << 32)]
            if results:
                rw[i] = [res[i]["len"], res[i]["lead"], res[i]["n_entries"] | (res[i]["status"] << 32), 0]
            c["carry"] = k
        o = self.tab["summary"]
        self.image[o:o + 64] = as_array(bytes(_lib.InboxSummary(**summ)))
        return res, summ, rows

    def where(self, o):
        for i in range(self.n):
            if self.offs[i] <= o < self.offs[i] + self.conns[i]["cap"]:
                return "range %d + %d" % (i, o - self.offs[i])
        for name, start in sorted(self.tab.items(), key=lambda kv: -kv[1]):
            if o >= start:
                return "%s + %d" % (name, o - start)
        return "in front of the ranges"

    def sweep(self, ctx, entries, pack=b"", m_cap=None, head_m=None, pack_len=None, pack_cap=None, pack_mis=0,
              pinned=False, stream=None, results=True, what="", check=True):
        m_cap = len(entries) if m_cap is None else m_cap
        head_m = len(entries) if head_m is None else head_m
        pack_len = len(pack) if pack_len is None else pack_len
        pack_cap = len(pack) if pack_cap is None else pack_cap
        ts, ps, imgs, full = self.inputs(entries, pack, m_cap, head_m, pack_len, pack_mis, pinned)
        need = _lib.load().xyws_inbox_scratch_bytes(self.n, m_cap)
        scratch = torch.full((need + PAD,), GUARD, dtype=torch.uint8, device="cuda")
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        o = self.tab
        torch.cuda.current_stream().synchronize()   # (the fills and uploads above ran on the current stream)
        rc = ctx.L.xyws_inbox_streams(ctx.h, vp(self.iconn_t), self.n, C.c_void_p(ps[0]),
                                      C.c_void_p(ps[1]) if m_cap else None, m_cap,
                                      C.c_void_p(ps[2]) if pack_cap else None, pack_cap,
                                      C.c_void_p(self.base + o["results"]) if results else None,
                                      C.c_void_p(self.base + o["summary"]), vp(scratch), need, s)
        assert rc == 0, what
        out = self.expect(full, pack, m_cap, head_m, pack_len, pack_cap, results)
        self.pending.append((ts, imgs, scratch, need, what))   # (alive until the stream has passed the call)
        if check:
            self.check()
        return out

    def check(self):
        torch.cuda.synchronize()
        ts, imgs, scratch, need, what = self.pending[-1]
        del self.pending[:-1]
        got = download(self.t)
        if got.tobytes() != self.image.tobytes():
            bad = int(np.flatnonzero(got != self.image)[0])
            raise AssertionError((what, self.where(bad), "got", int(got[bad]), "want", int(self.image[bad])))
        assert download(self.iconn_t).tobytes() == self.iconn_image.tobytes(), (what, "the iconn table changed")
        for name, t, img in zip(("head", "entries", "pack"), ts, imgs):
            got = t.numpy() if t.device.type == "cpu" else download(t)
            assert got.tobytes() == img.tobytes(), (what, name, "changed")
        assert bool((scratch[need:] == GUARD).all()), (what, "a byte behind the scratch changed")


def open_conns(caps, **kw):
    return [conn(c, flags=M.NO_HANDSHAKE, **kw) for c in caps]


# --------------------------------------------------------------------------- 1. seams
def test_connection_seams(ctx):
    """n at the tile's seams and one step beyond what the clear pass's grid covers."""
    T, S, GX, GY, EG = geometry()
    beyond = (EG * T - 8) // 4 + 1   # accumulator words behind the globals: four per connection
    for n in (1, T - 1, T, T + 1, 2 * T + 1, beyond + 1):
        pk, es, caps = Pack(), [], []
        for i in range(n):
            ln = 0 if i % 3 == 1 else 1 + (5 * i) % 7
            caps.append(ln + (i % 2))
            if ln:
                es.append(ent(i, pk.add(payload(i, ln)), ln, 0))
        es.reverse()
        w = World(open_conns(caps))
        res, summ, rows = w.sweep(ctx, es, pk.b, what=("n", n))
        assert summ["n_conns"] == len(es) and summ["bytes"] == sum(e["len"] for e in es)
        assert rows[n - 1]["conn_len"] == res[n - 1]["len"] == (0 if (n - 1) % 3 == 1 else 1 + (5 * (n - 1)) % 7)


def test_entry_seams(ctx):
    """M at the tile's seams, one step beyond the copy pass's grid and one beyond the entry pass's."""
    T, S, GX, GY, EG = geometry()
    n = 7
    for m in (1, T - 1, T, T + 1, GX + 1, EG * T + 1):
        pk, es, at = Pack(), [], [0] * n
        for k in range(m):
            c, ln = (k * 5) % n, k % 4
            es.append(ent(c, pk.add(payload(k, ln)), ln, at[c]))
            at[c] += ln
        w = World(open_conns([a + 3 for a in at]))
        res, summ, rows = w.sweep(ctx, es, pk.b, what=("m", m))
        assert summ["n_entries"] == m and summ["bytes"] == sum(at) and [r["len"] for r in res] == at
        assert sum(r["n_entries"] for r in res) == m and summ["status"] == 0


# --------------------------------------------------------------------------- 2. lengths and alignment
@pytest.mark.parametrize("apart", [True, False])
def test_lengths_and_alignments(ctx, apart):
    """Every length class at every destination residue, the source at the same
    residue and 1, 8 and 15 beyond it; ranges apart (each at its residue) or
    abutting (each an exact fit, so neighbours share their edge lines)."""
    S = geometry()[1]
    conns, es, pk = [], [], Pack()
    for ln in (0, 1, 15, 16, 17, S - 1, S, S + 1, 2 * S + 5):
        for r in range(16):
            for d in (0, 1, 8, 15):
                i = len(conns)
                conns.append(conn(ln, flags=M.NO_HANDSHAKE, mis=r if apart else None))
                es.append(ent(i, pk.add(payload(i, ln), (r + d) % 16), ln, 0))
    w = World(conns, apart=apart)
    if apart:
        assert all((w.base + w.offs[i]) % 16 == c["mis"] for i, c in enumerate(conns))
    else:
        assert all(w.offs[i] + c["cap"] == w.offs[i + 1] for i, c in enumerate(conns[:-1]))
        assert len({(w.base + o) % 16 for o in w.offs}) == 16
    res, summ, rows = w.sweep(ctx, es, pk.b)   # (the pack begins at a multiple of 16: `off` is the source residue)
    assert summ["bytes"] == sum(c["cap"] for c in conns) and summ["n_broken"] == 0
    for i in (5, len(conns) - 1):
        assert w.range_bytes(i) == payload(i, conns[i]["cap"])


def test_an_entry_longer_than_one_pass_of_the_copy_grid(ctx):
    """One entry of more than grid y x step bytes, so a workgroup of the copy
    pass takes a second chunk of it: with one entry of capacity (the largest
    grid y) and with as many as the grid's x holds (a small grid y)."""
    T, S, GX, GY, EG = geometry()
    long = GY * S + S + 5
    for m_cap in (1, GX):
        data, tail = payload(m_cap, long), payload(3, 40)
        pk = Pack()
        es = [ent(1, pk.add(tail, 2), 40, long), ent(1, pk.add(data, 9), long, 0), ent(0, pk.add(tail, 7), 40, 0)]
        w = World([conn(40, flags=M.NO_HANDSHAKE, mis=11), conn(long + 40, flags=M.NO_HANDSHAKE, mis=5),
                   conn(8, flags=M.NO_HANDSHAKE)])
        res, summ, rows = w.sweep(ctx, es, pk.b, m_cap=max(m_cap, 3), what=("m_cap", m_cap))
        assert w.range_bytes(1) == data + tail and w.range_bytes(0) == tail and summ["bytes"] == long + 80


# --------------------------------------------------------------------------- 3. several entries per connection
def test_interleaved_entries_out_of_order(ctx):
    """3 connections x 4 entries, interleaved with each other and listed out of `at` order."""
    S = geometry()[1]
    lens = [[5, 0, S + 3, 17], [16, 16, 1, 2 * S], [1, 2, 3, 4]]
    pk, es, want = Pack(), [], []
    for c, ls in enumerate(lens):
        at, whole = 0, b""
        for k, ln in enumerate(ls):
            data = payload(10 * c + k, ln)
            es.append(ent(c, pk.add(data, (3 * c + 5 * k) % 16), ln, at))
            at += ln
            whole += data
        want.append(whole)
    order = [11, 2, 7, 0, 9, 5, 4, 1, 10, 6, 3, 8]
    es = [es[k] for k in order]
    w = World(open_conns([len(x) + 2 for x in want]))
    res, summ, rows = w.sweep(ctx, es, pk.b)
    for c in range(3):
        assert w.range_bytes(c, len(want[c])) == want[c] and res[c]["n_entries"] == 4
    assert summ["n_entries"] == 12 and summ["n_conns"] == 3


# --------------------------------------------------------------------------- 4. every state path
def test_state_paths_over_four_sweeps(ctx):
    """Hand-written accept rows between the sweeps, as xyws_accept_streams would leave them."""
    R = 40  # bytes of a request
    req = payload(77, R)
    conns = [conn(100), conn(100), conn(100), conn(100), conn(100, flags=M.NO_HANDSHAKE),
             conn(100, flags=M.NO_HANDSHAKE), conn(100, flags=M.NO_HANDSHAKE), conn(100, null_rows=True)]
    w = World(conns)

    def sweep(items, what):
        """items: (conn, bytes, flags) in list order; `at` counts per connection."""
        pk, es, at = Pack(), [], {}
        for c, data, flags in items:
            es.append(ent(c, pk.add(data), len(data), at.get(c, 0), flags))
            at[c] = at.get(c, 0) + len(data)
        return w.sweep(ctx, es, pk.b, what=what)

    f = [payload(k, 9) for k in range(8)]
    # sweep 1: requests arrive: whole (0), the first half (1), whole with 5 frame bytes behind it (2), whole (3)
    res, summ, rows = sweep([(0, req, 0), (1, req[:17], 0), (2, req + f[2][:5], 0), (3, req, 0), (4, f[4], 0),
                             (7, req[:8], 0)], "sweep 1")
    assert [r["aconn_len"] for r in rows[:4]] == [R, 17, R + 5, R] and all(r["conn_len"] == 0 for r in rows[:4])
    assert rows[4] == dict(conn_off=0, conn_len=9, aconn_len=0) and summ["n_opened"] == 0
    w.set_aresult(0, M.ACC_ACCEPTED, R)
    w.set_aresult(2, M.ACC_ACCEPTED, R)
    w.set_aresult(3, M.ACC_REJECTED, R)
    # sweep 2: 0 opens without kept bytes, 2 with; 3 is refused; 1 gets its second half; 5 and 6 reach EOF
    res, summ, rows = sweep([(2, f[2][5:], 0), (0, f[0], 0), (1, req[17:], 0), (3, f[3], 0), (5, f[5], M.EOF_E),
                             (6, b"", M.EOF_E)], "sweep 2")
    assert rows[0] == dict(conn_off=0, conn_len=9, aconn_len=0) and res[0]["status"] == M.R_OPENED
    assert rows[2] == dict(conn_off=R, conn_len=9, aconn_len=0) and res[2]["lead"] == R
    assert w.range_bytes(2, R + 9) == req + f[2] and w.range_bytes(0, 9) == f[0]
    assert rows[1]["aconn_len"] == R and w.range_bytes(1, R) == req
    assert res[3]["status"] == M.R_REFUSED | M.R_DROPPED and w.range_bytes(3, R) == req
    assert res[5]["status"] == res[6]["status"] == M.R_EOF and (res[5]["len"], res[6]["len"]) == (9, 0)
    assert rows[4] == dict(conn_off=0, conn_len=0, aconn_len=0)       # idle after an active sweep
    assert (summ["n_opened"], summ["n_eof"], summ["n_broken"]) == (2, 2, 0)
    w.set_aresult(0, 0, 0)   # (accept over len 0: incomplete)
    w.set_aresult(2, 0, 0)
    w.set_aresult(1, M.ACC_ACCEPTED, R)
    # sweep 3: 1 opens without an entry; 0 and 2 receive at the front of their ranges; 3 stays dropped
    res, summ, rows = sweep([(0, f[1], 0), (2, f[6], 0), (3, f[3], 0)], "sweep 3")
    assert res[1]["status"] == M.R_OPENED and rows[1] == dict(conn_off=0, conn_len=0, aconn_len=0)
    assert rows[2] == dict(conn_off=0, conn_len=9, aconn_len=0) and w.range_bytes(2, 9) == f[6]
    assert res[3]["status"] == M.R_REFUSED | M.R_DROPPED and res[5]["status"] == M.R_EOF
    # sweep 4: everything idle but 1 and 7 (which has no rows and stays in HTTP state)
    res, summ, rows = sweep([(1, f[7], 0), (7, req[8:], 0)], "sweep 4")
    assert rows[1] == dict(conn_off=0, conn_len=9, aconn_len=0)
    assert all(r == dict(conn_off=0, conn_len=0, aconn_len=0) for k, r in enumerate(rows) if k not in (1, 7))
    assert w.conns[7]["carry"]["http_len"] == R and w.range_bytes(7, R) == req
    assert [c["carry"]["state"] for c in w.conns] == [M.OPEN, M.OPEN, M.OPEN, M.DEAD, M.OPEN, M.OPEN, M.OPEN, M.HTTP]


# --------------------------------------------------------------------------- 5. every fault
def test_faults_and_their_neighbours(ctx):
    http = lambda n: dict(http_len=n, bytes_total=n, state=M.HTTP, status=0)
    conns = [conn(32, flags=M.NO_HANDSHAKE),                                            # 0: a good neighbour
             conn(32, flags=M.NO_HANDSHAKE),                                            # 1: a bad range
             conn(32, flags=M.NO_HANDSHAKE),                                            # 2: a good neighbour
             conn(32, flags=M.NO_HANDSHAKE),                                            # 3: S != T (a gap)
             conn(64, carry=http(60)),                                                  # 4: an exact fit
             conn(64, carry=http(60)),                                                  # 5: overflow by one byte
             conn(64, carry=http(30), aresult=dict(status=M.ACC_ACCEPTED, consumed=31)),  # 6: consumed > http_len
             conn(32, flags=M.NO_HANDSHAKE)]                                            # 7: a good neighbour
    w = World(conns)
    pk = Pack()
    d = [payload(k, 8) for k in range(12)]
    es = [ent(0, pk.add(d[0]), 8, 0), ent(99, pk.add(d[1]), 8, 0), ent(1, pk.add(d[2]), 8, 0),
          ent(1, 1 << 40, 8, 8), ent(2, pk.add(d[3]), 8, 0), ent(3, pk.add(d[4]), 8, 0), ent(3, pk.add(d[5]), 8, 9),
          ent(4, pk.add(d[6][:4]), 4, 0), ent(5, pk.add(d[7][:5]), 5, 0), ent(6, pk.add(d[8]), 8, 0),
          ent(7, pk.add(d[9]), 8, 0), ent(8, 0, 1, 0)]
    res, summ, rows = w.sweep(ctx, es, pk.b, what="faults")
    assert [r["status"] for r in res] == [0, M.R_BAD_RANGE, 0, M.R_BAD_TILING, 0, M.R_OVERFLOW, M.R_BAD_CONSUMED, 0]
    assert [r["len"] for r in res] == [8, 0, 8, 0, 4, 0, 0, 8]
    assert (summ["n_bad_entries"], summ["n_broken"], summ["bytes"]) == (3, 4, 28)
    assert summ["status"] == M.S_BAD_ENTRIES | M.S_BROKEN
    for k in (1, 3, 5, 6):
        assert w.range_bytes(k) == bytes([GUARD]) * conns[k]["cap"] and w.conns[k]["carry"]["state"] == M.DEAD
    assert w.conns[4]["carry"]["http_len"] == 64
    # the next sweep: the broken ones stay dropped, their neighbours go on
    pk = Pack()
    es = [ent(k, pk.add(d[k]), 8, 0) for k in (0, 1, 2, 3, 5, 6, 7)]
    res, summ, rows = w.sweep(ctx, es, pk.b, what="the sweep after")
    assert [bool(r["status"] & M.R_DROPPED) for r in res] == [False, True, False, True, False, True, True, False]
    assert summ["n_broken"] == 0 and summ["bytes"] == 24 and w.range_bytes(1) == bytes([GUARD]) * 32


def test_entries_behind_the_head_and_a_head_above_m_cap(ctx):
    pk = Pack()
    d = [payload(k, 6) for k in range(4)]
    es = [ent(k, pk.add(d[k]), 6, 0) for k in range(4)]
    # head.m = 2 of 4 listed entries (and the poison behind them) are read
    w = World(open_conns([16] * 4))
    res, summ, rows = w.sweep(ctx, es, pk.b, head_m=2, what="head.m below the list")
    assert [r["len"] for r in res] == [6, 6, 0, 0] and summ["n_entries"] == 2 and summ["status"] == 0
    # head.m far above m_cap: clipped at m_cap, the row behind it is not read
    w = World(open_conns([16] * 4))
    res, summ, rows = w.sweep(ctx, es, pk.b, head_m=(1 << 40) + 3, what="head.m above m_cap")
    assert summ["n_entries"] == 4 and summ["status"] == M.S_CLIPPED and res[0]["status"] == 0
    # head.pack_len above pack_cap: the pack ends at pack_cap
    w = World(open_conns([16] * 4))
    res, summ, rows = w.sweep(ctx, es, pk.b, pack_len=1 << 50, pack_cap=17, what="pack_len above pack_cap")
    assert [r["status"] for r in res] == [0, 0, M.R_BAD_RANGE, M.R_BAD_RANGE] and summ["bytes"] == 12


# --------------------------------------------------------------------------- 6. call mechanics
def some_sweep(n, seed):
    rng = random.Random(seed)
    pk, es, caps = Pack(), [], []
    for i in range(n):
        at = 0
        for k in range(rng.randint(0, 3)):
            ln = rng.choice([0, 3, 16, 40, 1100])
            es.append(ent(i, pk.add(payload(seed + 3 * i + k, ln), rng.randrange(16)), ln, at))
            at += ln
        caps.append(at + rng.randint(0, 2))
    rng.shuffle(es)
    return caps, es, pk.b


def test_same_call_twice_on_restored_carries(ctx):
    caps, es, pack = some_sweep(40, 5)
    w = World(open_conns(caps))
    w.sweep(ctx, es, pack, what="first")
    first = download(w.t).copy()
    # the carries back to fresh, the ranges to guards: the same call writes the same bytes
    w2 = World(open_conns(caps))
    w.t.copy_(w2.t)
    w.image[:] = w2.image
    for c in w.conns:
        c["carry"] = None
    w.sweep(ctx, es, pack, what="second")
    second = download(w.t)
    assert first.tobytes() == second.tobytes()


def test_two_streams_at_once(ctx):
    worlds, sweeps = [], []
    for seed in (1, 2):
        caps, es, pack = some_sweep(300, seed)
        worlds.append(World(open_conns(caps)))
        sweeps.append((es, pack))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):   # three sweeps each, issued in turn: the calls of the two streams overlap
        for w, (es, pack), s in zip(worlds, sweeps, streams):
            w.sweep(ctx, es, pack, stream=s.cuda_stream, check=False, what="two streams")
        for w in worlds:
            w.check()


def test_no_entries_and_no_connections(ctx):
    # M = 0: every connection idle; a stale length goes back to 0, the summary is written
    w = World(open_conns([8, 8, 8]))
    res, summ, rows = w.sweep(ctx, [ent(1, 0, 4, 0)], payload(1, 4), what="one entry")
    assert rows[1]["conn_len"] == 4
    res, summ, rows = w.sweep(ctx, [], b"", what="M = 0")
    assert summ == dict(n_entries=0, bytes=0, n_conns=0, n_opened=0, n_eof=0, n_broken=0, n_bad_entries=0, status=0)
    assert rows[1]["conn_len"] == 0
    res, summ, rows = w.sweep(ctx, [], b"", m_cap=5, what="M = 0 of 5")      # (the poison rows are not read)
    assert summ["n_entries"] == 0
    res, summ, rows = w.sweep(ctx, [ent(0, 0, 2, 0)], payload(2, 2), results=False, what="no result table")
    assert rows[0]["conn_len"] == 2
    # n = 0: OK, nothing launched, nothing written
    g = torch.full((256,), GUARD, dtype=torch.uint8, device="cuda")
    assert ctx.L.xyws_inbox_streams(ctx.h, vp(g), 0, vp(g), vp(g), 1, vp(g), 16, vp(g), vp(g), vp(g), 256, None) == 0
    torch.cuda.synchronize()
    assert bool((g == GUARD).all())


# --------------------------------------------------------------------------- 7. pinned sources
def test_pinned_sources_equal_device_sources(ctx):
    caps, es, pack = some_sweep(300, 9)
    dev, pin = World(open_conns(caps)), World(open_conns(caps))
    dev.sweep(ctx, es, pack, pack_mis=5, what="device")
    pin.sweep(ctx, es, pack, pack_mis=5, pinned=True, what="pinned")
    a, b = download(dev.t), download(pin.t)
    lo, hi = dev.tab["conns"], dev.tab["carries"]     # (the rows hold addresses of their own image)
    assert a[:lo].tobytes() == b[:lo].tobytes() and a[hi:].tobytes() == b[hi:].tobytes()


# --------------------------------------------------------------------------- 8. the real calls
def frame(data, key, op=0x82):
    n = len(data)
    head = bytes([op, 0x80 | n]) if n < 126 else bytes([op, 0x80 | 126, n >> 8, n & 255])
    return head + key + bytes(b ^ key[k % 4] for k, b in enumerate(data))


class Rig:
    """n slot-stable connections with everything a sweep of xyws_inbox_streams,
    xyws_accept_streams and xyws_decode_streams needs, in one arena; head,
    entries and pack are fixed buffers that load() rewrites."""
    FCAP, RESP = 8, 144

    def __init__(self, ctx, n, recv_cap, m_cap, pack_cap, no_handshake=()):
        self.ctx, self.n, self.recv_cap, self.m_cap, self.pack_cap = ctx, n, recv_cap, m_cap, pack_cap
        p, self.at = 64 + 5, {}
        for name, size in (("slab", n * recv_cap), ("conns", 64 * n), ("aconns", 32 * n), ("aresults", 32 * n),
                           ("icarries", 32 * n), ("dcarries", 64 * n), ("frames", 32 * self.FCAP * n), ("counts", 8 * n),
                           ("resp", self.RESP * n), ("results", 32 * n), ("summary", 64)):
            self.at[name] = p
            p = (p + size + PAD + 63) & ~63
        self.arena = torch.zeros(p, dtype=torch.uint8, device="cuda")
        b, at = ptr(self.arena), self.at
        self.base = b
        conns, aconns, iconns = np.zeros((n, 8), np.uint64), np.zeros((n, 4), np.uint64), np.zeros((n, 8), np.uint64)
        for i in range(n):
            buf = b + at["slab"] + recv_cap * i
            conns[i, :5] = [buf, 0, b + at["dcarries"] + 64 * i, b + at["frames"] + 32 * self.FCAP * i, self.FCAP]
            aconns[i] = [buf, 0, b + at["resp"] + self.RESP * i, self.RESP]
            iconns[i] = [buf, recv_cap, b + at["icarries"] + 32 * i, b + at["conns"] + 64 * i, b + at["aconns"] + 32 * i,
                         b + at["aresults"] + 32 * i, M.NO_HANDSHAKE if i in no_handshake else 0, 0]
        self.put("conns", conns)
        self.put("aconns", aconns)
        self.iconns = upload(iconns.reshape(-1).view(np.uint8))
        self.head = torch.zeros(32, dtype=torch.uint8, device="cuda")
        self.entries = torch.zeros(32 * m_cap, dtype=torch.uint8, device="cuda")
        self.pack = torch.zeros(pack_cap, dtype=torch.uint8, device="cuda")
        self.need = ctx.L.xyws_inbox_scratch_bytes(n, m_cap)
        self.scratch = torch.zeros(self.need, dtype=torch.uint8, device="cuda")

    def put(self, name, a):
        raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        self.arena[self.at[name]:self.at[name] + raw.size].copy_(upload(raw))

    def load(self, entries, pack):
        """Only the head, the entries and the pack are rewritten between two sweeps."""
        assert len(entries) <= self.m_cap and len(pack) <= self.pack_cap
        self.head.copy_(upload(np.array([len(entries), len(pack), 0, 0], np.uint64).view(np.uint8)))
        if entries:
            self.entries[:32 * len(entries)].copy_(upload(entries_image(entries, len(entries))))
        if len(pack):
            self.pack[:len(pack)].copy_(upload(as_array(bytes(pack))))

    def run(self, stream=None):
        L, h, b, at, n = self.ctx.L, self.ctx.h, self.base, self.at, self.n
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        assert L.xyws_inbox_streams(h, vp(self.iconns), n, vp(self.head), vp(self.entries), self.m_cap, vp(self.pack),
                                    self.pack_cap, C.c_void_p(b + at["results"]), C.c_void_p(b + at["summary"]),
                                    vp(self.scratch), self.need, s) == 0
        assert L.xyws_accept_streams(h, C.c_void_p(b + at["aconns"]), n, 1024, 0, C.c_void_p(b + at["aresults"]), s) == 0
        assert L.xyws_decode_streams(h, C.c_void_p(b + at["conns"]), n, C.c_void_p(b + at["counts"]), 0, s) == 0

    def rows(self, snap, name, struct):
        size = C.sizeof(struct)
        raw = snap[self.at[name]:self.at[name] + size * self.n].tobytes()
        return [struct.from_buffer_copy(raw, size * k) for k in range(self.n)]


def test_the_invariant_with_the_real_calls(ws, ctx):
    """Rule 10: streams of a request and 3 to 5 masked frames of 0 to 300 bytes,
    cut by a seeded generator into 4 sweeps of 0 to 3 entries per connection (and
    a fifth sweep without entries, in which a request that ended in the fourth
    opens), against xyws_accept_request and xyws_decode_stream fed the same
    pieces one connection at a time."""
    from test_gpu_roster import request
    rng = random.Random(20261021)
    n, SWEEPS = 6, 4
    streams, reqs = [], []
    for i in range(n):
        req = request(b"dGhlIHNhbXBsZSBub25jZQ==") if i != 3 else request(b"dGhlIHNhbXBsZSBub25jZQ==").replace(b"13", b"12")
        fr = b"".join(frame(payload(31 * i + k, rng.choice([0, 1, 125, 126, 300, rng.randint(0, 300)])),
                            bytes(rng.randrange(256) for _ in range(4)), 0x82 if k else 0x81)
                      for k in range(rng.randint(3, 5)))
        reqs.append(req)
        streams.append(req + fr)
    rig = Rig(ctx, n, recv_cap=2048, m_cap=3 * n, pack_cap=16384)
    # per connection: how many entries each sweep brings, and where they cut its stream
    plan = []
    for i in range(n):
        ks = [rng.randint(0, 3) for _ in range(SWEEPS)]
        if not any(ks):
            ks[rng.randrange(SWEEPS)] = 1
        runs = iter(M.cut(len(streams[i]), sum(1 for k in ks if k), rng))
        plan.append([M.cut(next(runs), k, rng) if k else [] for k in ks])
    pos = [0] * n
    chunks = [[] for _ in range(n)]       # what xyws_decode_streams saw of each connection, sweep by sweep
    verdict = [None] * n
    for s in range(SWEEPS + 1):
        pk, es = Pack(), []
        for i in range(n):
            at = 0
            for ln in (plan[i][s] if s < SWEEPS else []):
                es.append((i, streams[i][pos[i]:pos[i] + ln], at))
                at += ln
                pos[i] += ln
        rng.shuffle(es)
        es = [ent(i, pk.add(data, rng.randrange(16)), len(data), at) for i, data, at in es]
        rig.load(es, pk.b)
        rig.run()
        torch.cuda.synchronize()
        snap = download(rig.arena)
        ares, crow = rig.rows(snap, "aresults", _lib.AcceptResult), rig.rows(snap, "conns", _lib.Conn)
        counts = snap[rig.at["counts"]:rig.at["counts"] + 8 * n].view(np.uint64)
        for i in range(n):
            if ares[i].status & (M.ACC_ACCEPTED | M.ACC_REJECTED) and verdict[i] is None:
                verdict[i] = (bytes(ares[i]), snap[rig.at["resp"] + rig.RESP * i:][:ares[i].resp_len].tobytes())
            if crow[i].len:
                o = crow[i].buf - rig.base
                fo = rig.at["frames"] + 32 * rig.FCAP * i
                # the bytes as the inbox placed them are those of the stream; after the decode they are unmasked
                chunks[i].append((int(crow[i].len), snap[o:o + crow[i].len].tobytes(), int(counts[i]),
                                  snap[fo:fo + 32 * min(int(counts[i]), rig.FCAP)].tobytes()))
            else:
                assert counts[i] == 0
    assert pos == [len(x) for x in streams]
    final = download(rig.arena)
    for i in range(n):
        # the verdict: xyws_accept_request on the request alone
        res, out = _lib.AcceptResult(), C.create_string_buffer(rig.RESP)
        assert ctx.L.xyws_accept_request(reqs[i], len(reqs[i]), 1024, 0, out, rig.RESP, C.byref(res)) == 0
        assert verdict[i] is not None and verdict[i][0] == bytes(res), i
        assert verdict[i][1] == out.raw[:res.resp_len], i
        if i == 3:
            assert res.status & M.ACC_REJECTED and not chunks[i]
            continue
        assert res.status & M.ACC_ACCEPTED and res.consumed == len(reqs[i])
        # the frames: xyws_decode_stream over the bytes behind `consumed`, piece by piece as the sweeps brought them
        behind = streams[i][res.consumed:]
        assert sum(c[0] for c in chunks[i]) == len(behind), i
        dec, p = ws.frame_decoder(ctx=ctx), 0
        for ln, got, cnt, frames in chunks[i]:
            t = upload(as_array(behind[p:p + ln]))
            r = dec.decode(t, cap=rig.FCAP)
            torch.cuda.synchronize()
            assert download(t).tobytes() == got, (i, p)
            assert r.nframes == cnt and download(r.frames_t)[:len(frames)].tobytes() == frames, (i, p)
            p += ln
        o = rig.at["dcarries"] + 64 * i
        assert final[o:o + 64].tobytes() == download(dec.carry_t).tobytes(), i
        assert dec.carry().payload_remaining == 0


# --------------------------------------------------------------------------- 9. one graph, sweeps of any shape
def test_one_captured_graph_serves_three_different_sweeps(ctx):
    """inbox, accept and decode captured once with m_cap = 16; between two
    replays only the head, the entries and the pack are rewritten. The sweeps
    differ in who receives and how much, and the second opens a connection;
    each replay leaves the arena as the direct run of the same inputs did."""
    from test_gpu_roster import request
    req = request(b"dGhlIHNhbXBsZSBub25jZQ==")
    f = [frame(payload(k, 20 + 30 * k), bytes([k + 1, 2, 3, 4])) for k in range(5)]
    sweeps = []
    for items in ([(0, req + f[0][:3]), (1, req[:50]), (2, f[1])],
                  [(1, req[50:]), (0, f[0][3:] + f[2]), (2, f[3][:10]), (0, f[4][:1])],
                  [(2, f[3][10:]), (3, req), (1, f[4])]):
        pk, es, at = Pack(), [], {}
        for c, data in items:
            es.append(ent(c, pk.add(data, 7), len(data), at.get(c, 0)))
            at[c] = at.get(c, 0) + len(data)
        sweeps.append((es, pk.b))
    rig = Rig(ctx, 4, recv_cap=512, m_cap=16, pack_cap=1024, no_handshake=(2,))
    start = rig.arena.clone()
    direct = []
    for es, pack in sweeps:
        rig.load(es, pack)
        rig.run()
        torch.cuda.synchronize()
        direct.append(download(rig.arena).copy())
    res = [rig.rows(d, "results", _lib.InboxResult) for d in direct]
    assert res[1][0].status & M.R_OPENED and res[2][1].status & M.R_OPENED and not res[0][0].status
    assert [r.len for r in res[1]] == [len(f[0]) - 3 + len(f[2]) + 1, len(req) - 50, 10, 0]
    counts = [d[rig.at["counts"]:rig.at["counts"] + 32].view(np.uint64).tolist() for d in direct]
    assert counts[0][:3] == [0, 0, 1] and counts[1][0] >= 2 and counts[2][1] == 1 and counts[2][3] == 0
    rig.arena.copy_(start)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    rig.load(*sweeps[0])
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        rig.run(stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert download(rig.arena).tobytes() == download(start).tobytes()   # (capture ran nothing)
    for k, (es, pack) in enumerate(sweeps):
        rig.load(es, pack)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        got = download(rig.arena)
        if got.tobytes() != direct[k].tobytes():
            bad = int(np.flatnonzero(got != direct[k])[0])
            raise AssertionError(("replay", k, "arena byte", bad, "got", int(got[bad]), "want", int(direct[k][bad])))


# --------------------------------------------------------------------------- 10. connection_group.inbox
def test_connection_group_inbox_and_its_refusals(ws, ctx):
    from test_gpu_roster import masked, request, response
    key = b"dGhlIHNhbXBsZSBub25jZQ=="
    req, hello = request(key), masked(b"hello")
    grp, other = ws.connection_group(3, cap=4, ctx=ctx), ws.connection_group(3, cap=4, ctx=ctx)
    with pytest.raises(_lib.XywsError):
        grp.inbox(req, [(0, 0, len(req), 0)], recv_cap=0)
    with pytest.raises(_lib.XywsError):
        grp.inbox(req, [(0, 0, len(req))], recv_cap=512)            # (an entry lacks `at`)
    with pytest.raises(_lib.XywsError):
        grp.inbox(req, [(0, 0, -1, 0)], recv_cap=512)
    with pytest.raises(_lib.XywsError):
        grp.inbox(req, [(0, 0, 1, 0), (0, 1, 1, 1)], recv_cap=512, m_cap=1)
    with pytest.raises(_lib.XywsError):
        grp.inbox(torch.zeros(4, dtype=torch.uint8), [], recv_cap=512)  # (a pack in host memory)
    # sweep 1: connection 1 sends its request in two entries with the first frame bytes behind it
    cut = 30
    ib = grp.inbox(req + hello[:4], [(1, cut, len(req) - cut + 4, cut), (1, 0, cut, 0)], recv_cap=512)
    with pytest.raises(_lib.XywsError):
        grp.inbox(req, [], recv_cap=256)                             # (recv_cap is fixed by the first call)
    with pytest.raises(_lib.XywsError):
        other.decode(ib)
    with pytest.raises(_lib.XywsError):
        other.accept(ib, None)
    with pytest.raises(_lib.XywsError):
        grp.accept(ib, [torch.zeros(144, dtype=torch.uint8, device="cuda")])
    acc, dec = grp.accept(ib, None), grp.decode(ib)
    s = ib.summary()
    assert (s.n_entries, s.bytes, s.n_conns, s.n_opened, s.status) == (2, len(req) + 4, 1, 0, 0)
    assert ib.result(1).len == len(req) + 4 and ib.result(0).n_entries == 0
    assert acc.result(1).status & _lib.ACC_ACCEPTED and acc.result(1).consumed == len(req)
    assert acc.response(1) == response(key) and not acc.result(0).status
    assert [dec.nframes(k) for k in range(3)] == [0, 0, 0]
    assert grp.inbox_carry(1).http_len == len(req) + 4 and grp.inbox_carry(1).state == _lib.IB_HTTP
    # sweep 2: it opens; the kept bytes and the new ones are one decode input; connection 0 says something unasked
    ib = grp.inbox(hello[4:] + b"junk", [(1, 0, len(hello) - 4, 0), (0, len(hello) - 4, 4, 0)], recv_cap=512)
    acc, dec = grp.accept(ib, None), grp.decode(ib)
    r = ib.result(1)
    assert r.status == _lib.IBR_OPENED and r.lead == len(req) and ib.summary().n_opened == 1
    assert ib.conn(1).len == len(hello) and dec.nframes(1) == 1 and dec.nframes(0) == 0
    assert ib.received(1)[6:] == b"hello" and dec.frames(1)[0].payload_len == 5
    assert grp.inbox_carry(1).state == _lib.IB_OPEN and grp.inbox_carry(0).http_len == 4
    assert not acc.result(1).status                                  # (len 0: incomplete, nothing is sent twice)
    # reset() gives the slot to a new connection: its inbox carry is fresh again
    grp.reset([1])
    c = grp.inbox_carry(1)
    assert (c.http_len, c.bytes_total, c.state, c.status) == (0, 0, _lib.IB_HTTP, 0) and grp.inbox_carry(0).http_len == 4
    grp.reset()
    assert grp.inbox_carry(0).http_len == 0


def test_a_slot_that_changes_hands_in_the_sweep_after_a_verdict(ws, ctx):
    """The sweep after a verdict is when a slot is normally recycled, and the
    slot's accept row still holds that verdict then: reset() clears it with the
    carry, so the new connection's request is placed and answered. Without the
    reset the row decides, as rule 3 says it does for the connection that sent it."""
    from test_gpu_roster import request, response
    key = b"dGhlIHNhbXBsZSBub25jZQ=="
    good = request(key)
    bad = good.replace(b"Version: 13", b"Version: 12")
    G, B = len(good), len(bad)
    grp, kept = ws.connection_group(2, cap=4, ctx=ctx), ws.connection_group(2, cap=4, ctx=ctx)

    def sweep(g, pieces):
        pack, es = b"", []
        for c, data in pieces:
            es.append((c, len(pack), len(data), 0))
            pack += data
        ib = g.inbox(pack, es, recv_cap=512)
        return ib, g.accept(ib, None), g.decode(ib)

    for g in (grp, kept):   # sweep k: connection 0 is refused, connection 1 accepted
        ib, acc, dec = sweep(g, [(0, bad), (1, good)])
        assert acc.result(0).status & _lib.ACC_REJECTED and acc.result(0).http_status == 426
        assert acc.result(1).status & _lib.ACC_ACCEPTED and acc.result(1).consumed == G
    # both peers are gone and the slots are given to new connections, which send their requests in sweep k + 1
    grp.reset([0, 1])
    ib, acc, dec = sweep(grp, [(1, good), (0, good)])
    assert ib.summary().n_broken == 0 and ib.summary().n_opened == 0 and ib.summary().bytes == 2 * G
    for k in (0, 1):
        r, c = ib.result(k), grp.inbox_carry(k)
        assert (r.len, r.lead, r.status) == (G, 0, 0), k
        assert (c.http_len, c.bytes_total, c.state, c.status) == (G, G, _lib.IB_HTTP, 0), k
        a = acc.result(k)
        assert a.status == _lib.ACC_ACCEPTED and a.consumed == G and acc.response(k) == response(key), k
        assert ib.conn(k).len == 0 and dec.nframes(k) == 0
    # the same with reset() of every slot, right after these two verdicts
    grp.reset()
    ib, acc, dec = sweep(grp, [(0, good)])
    assert (ib.result(0).len, ib.result(0).status, ib.result(1).status) == (G, 0, 0)
    assert acc.result(0).status == _lib.ACC_ACCEPTED and not acc.result(1).status
    assert grp.inbox_carry(1).state == _lib.IB_HTTP
    # the group that kept its connections: the rows of sweep k decide in sweep k + 1
    ib, acc, dec = sweep(kept, [(0, good), (1, b"")])
    assert ib.result(0).status == _lib.IBR_REFUSED | _lib.IBR_DROPPED and ib.result(0).len == 0
    assert ib.result(1).status == _lib.IBR_OPENED and kept.inbox_carry(0).state == _lib.IB_DEAD
