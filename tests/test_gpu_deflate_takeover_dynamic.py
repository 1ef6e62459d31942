"""xyws_deflate_windows_streams with XYWS_DFO_WINDOW_DYNAMIC. Reference: zlib's inflater over the history (test_gpu_deflate_takeover's
Call.check); no record is longer than the call with opts 0 makes it, nor than xyws_deflate_streams with XYWS_DFO_DYNAMIC (Both.check)."""
import random
import zlib

import pytest

import test_gpu_deflate_takeover as T
from test_gpu_deflate_dynamic import Dynamic, rnd
from test_gpu_deflate_takeover import CHAT, COMPLETE, END, HIST, STAGE, VM, WINDOW, Call, Room, chat, dev, frames_of, grp, ptr, torch  # noqa: F401
from xynet_amd import _lib

pytestmark = pytest.mark.gpu
noise = lambda n, seed: bytes(random.Random(seed).choices(b"abcdefgh", k=n))  # noqa: E731 (3 bits a byte)


class Both(Call):
    """Call with the bit. check() (rooms that all take over): and self.lens, the records' lengths here, with opts 0 over the same histories, with XYWS_DFO_DYNAMIC."""
    def run(self, g, stream=None):
        s, ro = self.s, ptr(self.roster) if self.roster is not None else None
        assert g.ctx.L.xyws_deflate_windows_streams(g.ctx.h, ptr(s.rt), ptr(s.rres), ptr(self.bconns), ptr(s.dt), s.n, ptr(self.rt),
                                                    ptr(self.dt), ro, len(self.rooms), _lib.DFO_WINDOW_DYNAMIC, ptr(s.view), ptr(s.vres),
                                                    ptr(s.vbc), ptr(s.res), ptr(self.rres), stream) == 0
        return self

    def check(self, g, **kw):
        s, before, kws = self.s, [r.hist for r in self.rooms], dict(out_caps=self.s.caps, vmsg_cap=self.s.vmsg_cap)
        rows, w, d = super().check(g, **kw), Call(s.conns, [Room().preset(h) for h in before], **kws).run(g), Dynamic(s.conns, **kws)
        d.deflate(g, self.bconns, None)
        self.lens = [[r.length for r in _lib.read_rows(_lib.Message, t.vmsgs, (VM + 1) * s.n)] for t in (s, w.s, d)]
        assert all(a <= b and a <= e for a, b, e in zip(*self.lens))
        return rows


@pytest.mark.parametrize("name, arg", [("test_shapes", 0), ("test_shapes", 1), ("test_shapes", HIST), ("test_shapes", WINDOW), ("test_captured_and_replayed", None)])
def test_the_sibling_s_tables_with_the_bit(grp, monkeypatch, name, arg):
    """Its shapes (eight lengths, heads of 0 and 7 bytes, odd offsets, a sweep over the slid history) and its graph replay, by Both."""
    monkeypatch.setattr(T, "Call", Both)
    getattr(T, name)(grp, *([] if arg is None else [arg]))


@pytest.mark.parametrize("hist", [noise(4096, 1), rnd(HIST, 3)], ids=["half_history_half_noise", "pieces_history_noise_random_then_a_random_record"])
def test_shorter_than_either_alone(grp, hist):
    """Only the window shortens what repeats the history, only a dynamic code 8-letter noise; a random record stays stored."""
    recs = [hist[1000:2024] + noise(1024, 2)] if len(hist) < HIST else [hist + noise(STAGE, 4) + rnd(5, 5), rnd(2 * STAGE + 5, 6)]
    c = Both([(b"", 0, [(m, COMPLETE, 1) for m in recs])], [Room().preset(hist)]).run(grp)
    row, r, (a, w, d) = c.check(grp)[0], _lib.read_rows(_lib.DeflateResult, c.s.res, 1, 0)[0], c.lens
    assert a[0] < w[0] and a[0] < d[0] and (row.n_history, r.n_dynamic, r.n_stored) == (1, 1, len(recs) - 1)
    assert len(recs) == 1 or a[1] == len(recs[1]) + 6


def test_mixed_table(grp):
    """A room with a null carry and a connection without a room are XYWS_DFO_DYNAMIC's byte for byte; a member beyond vmsg_cap; the guards (Call.check)."""
    conns = [(h, r, recs) for r in (0, 1) for h, _, recs in chat(0)] + [(b"n: ", _lib.ROOM_NONE, [(CHAT[0], COMPLETE, 1)]), (b"", 0, [(CHAT[k], COMPLETE, 1) for k in range(3)])]
    c, p = Both(conns, [Room(), Room(takeover="text")], vmsg_cap=2).run(grp), Dynamic(conns, vmsg_cap=2)
    assert Call.check(c, grp)[0].status == _lib.DFR_DESYNC and _lib.read_rows(_lib.DeflateResult, c.s.res, 1, 7)[0].status == _lib.DFL_MSG_CAP
    p.deflate(grp, c.bconns, None)
    for k in (3, 4, 5, 6):
        for a, b, lo, n in ((c.s.slab, p.slab, c.s.offs[k], c.s.caps[k]), (c.s.vbc, p.vbc, 64 * k, 64), (c.s.vres, p.vres, 32 * k, 32), (c.s.res, p.res, 32 * k, 32)):
            assert torch.equal(a[lo:lo + n], b[lo:lo + n]), k


def test_through_connection_group(grp):
    """grp.deflate(dynamic=True, takeover=[0]) into grp.broadcast(deflated=...): RSV1 frames that one inflater follows, the history."""
    import streams
    from xynet_amd import websocket as ws
    g, key, client, said = ws.connection_group(3, cap=8), b"\x37\xfa\x21\x3d", zlib.decompressobj(-15), [m for _, _, ((m, _, _),) in chat(0)]
    bufs = [dev(streams.header(0x81, len(m), key) + streams.masked(m, key)) for m in said]
    msgs = g.reassemble(g.decode(list(enumerate(bufs))), [torch.zeros(600, dtype=torch.uint8, device="cuda") for _ in range(3)])
    sends, want = [torch.zeros(2000, dtype=torch.uint8, device="cuda") for _ in range(3)], [(0xC1, b"%d: " % k + m) for k, m in enumerate(said)]
    dfl = g.deflate(msgs, [1], 400, dynamic=True, takeover=[0])
    bc = g.broadcast(msgs, [[0, 1, 2]], sends, heads=[dev(b"%d: " % k) for k in range(3)], deflated=dfl)
    sent = frames_of(sends[1][:bc.result(1).send_len].cpu().numpy().tobytes())
    assert [(b0, client.decompress(pay + END)) for b0, pay in sent] == want and sum(dfl.result(k).n_dynamic for k in range(3)) >= 1
    assert g.deflate_history(0).cpu().numpy().tobytes() == b"".join(p for _, p in want)
