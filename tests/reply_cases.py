"""Streams and cuts for the xyws_reply_streams tests (model and device)."""
import history
import msg_streams
import streams

MAX_PAYLOAD = 1 << 20


def echo_stream(seed, nframes, close=True, big=False):
    """A client stream an echo service sees: text and binary frames of all
    three length forms' sizes, pings and pongs, now and then (1 in 40) a frame
    the policy closes on (a fragment, an unmasked frame), and a close frame
    with a status code at the end."""
    rng = streams.SplitMix(seed)
    out = b""
    for _ in range(nframes):
        r = rng.below(40)
        n = [0, 1, 5, 125, 126, 127, 300][rng.below(7)] if rng.below(3) else rng.below(1001)
        if big and rng.below(8) == 0:
            n = 65536 + rng.below(100)
        if r == 0:
            out += streams.frame(rng, 0x01, n)  # FIN = 0
        elif r == 1:
            out += streams.frame(rng, 0x82, n, masked_frame=False)
        elif r < 6:
            out += streams.frame(rng, 0x89, rng.below(126))
        elif r < 8:
            out += streams.frame(rng, 0x8A, rng.below(20))
        else:
            out += streams.frame(rng, 0x81 if r & 1 else 0x82, n)
    if close:
        out += msg_streams.close_frame(rng, 1001, b"bye")
    return out


def random_cuts(rng, length, k):
    return sorted(rng.below(length + 1) for _ in range(k))


def header_cuts(wire, starts):
    """For the frame starts given, the cuts that split a header after each of
    its bytes: one list of cuts per (frame, byte)."""
    out = []
    for s in starts:
        b1 = wire[s + 1] & 0x7F
        h = 2 + (2 if b1 == 126 else 8 if b1 == 127 else 0) + (4 if wire[s + 1] & 0x80 else 0)
        out += [[s + k] for k in range(1, h + 1) if s + k <= len(wire)]
    return out


def frame_starts(oracle, wire):
    import reply_model as M
    fr, _, _ = oracle.decode_stream(M.as_array(wire))
    return [f.frame_off for f in fr]


def named_streams():
    """Stream kinds of the decode tests' split probes (history.SPLIT_NAMES)
    and a message stream with pings, each with a final close."""
    rng = streams.SplitMix(0xC105E)
    out = {}
    for name in ("lengths", "fragments", "trunc_hdr_9", "rsv_reserved_ops", "unmasked_mix", "nonminimal"):
        assert name in history.SPLIT_NAMES or name in streams.EDGE_CASES
        out[name] = streams.case_bytes(name) + msg_streams.close_frame(rng, 1000)
    out["messages"] = msg_streams.message_stream(0x5EED, nmsg=12)[0] + msg_streams.close_frame(rng, 1001, b"done")
    return out
