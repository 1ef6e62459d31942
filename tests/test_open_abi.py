"""CPU checks of xyws_open_streams' boundary: every refusal decided on the arguments alone (no device), n == 0,
xyws_directory_init's sizes and refusals, and tests/cpp/directory_host_check.cpp (a stand-alone program with its own
main, AddressSanitizer and UBSan linked into it) over xyws_directory.h on the host."""
import ctypes as C
import os
import subprocess

import pytest

import xynet_amd._lib as L


def test_streams_refusals_without_a_device():
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx = p = C.cast(fake, C.c_void_p)
    ok = dict(ac=p, rt=p, n=1, d=p, dl=4096, rc=p, nrc=1, res=p, work=p)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_open_streams(c, a["ac"], a["rt"], a["n"], a["d"], a["dl"], a["rc"], a["nrc"], 0, a["res"], a["work"],
                                     None)

    assert call(c=None) == -1 and call(c=None, n=0) == -1
    for name in ("ac", "rt", "res", "work", "d", "rc"):
        assert call(**{name: None}) == -1, name
    assert call(dl=0) == -1 and call(n=0xFFFFFFFF) == -1 and call(n=1 << 40) == -1
    assert call(n=0, d=None) == -1 and call(n=0, dl=0) == -1 and call(n=0, rc=None) == -1
    assert call(n=0) == 0 and call(n=0, ac=None, rt=None, res=None, work=None, rc=None, nrc=0) == 0


def init(slots, base, cap, keys_cap, room=1 << 16, blob=True):
    need, buf = C.c_uint64(0x1234), C.create_string_buffer(1 << 16)
    rc = L.load().xyws_directory_init(slots, base, cap, keys_cap, buf if blob else None, room, C.byref(need))
    return rc, need.value, buf.raw[:need.value]


def test_directory_init_sizes_and_refusals():
    rc, need, blob = init(0, 10, 4, 100)
    assert rc == 0 and need == 64 + 32 * 8 + 100 and blob[:4] == b"XYRD" and int.from_bytes(blob[4:8], "little") == 1
    assert init(0, 10, 4, 100)[2] == blob                                  # no pointer in it: two inits are equal bytes
    assert init(0, 10, 5, 0)[1] == 64 + 32 * 16 and init(64, 10, 5, 0)[1] == 64 + 32 * 64 and init(0, 0, 0, 0)[1] == 64 + 64
    assert all(init(slots, 10, 4, 100)[:2] == (-1, 0) for slots in (3, 4, 6, 12))  # no power of two, or < 2 * room_cap
    assert init(0, 0xFFFFFFFF, 1, 0)[:2] == (-1, 0) and init(0, 0xFFFFFFFE, 1, 0)[0] == 0  # XYWS_ROOM_NONE is no room
    assert init(0, 0, 1 << 30, 0)[:2] == (-1, 0) and init(0, 0, 4, 0xFFFFFFFF)[:2] == (-1, 0)  # 4 GiB or more
    # need is written whatever cap; nothing else is when it does not suffice
    assert init(8, 10, 4, 100, room=0)[:2] == (-4, need) and init(8, 10, 4, 100, room=need - 1)[:2] == (-4, need)
    assert init(8, 10, 4, 100, room=need)[0] == 0 and init(8, 10, 4, 100, blob=False)[0] == -1
    assert L.load().xyws_directory_init(8, 10, 4, 100, None, 0, None) == -4  # need is nullable
    with pytest.raises(L.XywsError):
        L.directory_blob(10, 4, slots=4)


def test_directory_host_side_under_sanitizers(tmp_path):
    exe, csrc = tmp_path / "directory_host_check", os.path.join(L.PKG, "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(L.ROOT, "include"), "-I", csrc,
                        os.path.join(L.ROOT, "tests", "cpp", "directory_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "0 failed", r.stdout[-2000:] + r.stderr[-4000:]
