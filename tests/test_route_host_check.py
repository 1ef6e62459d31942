"""The route table and its lookup under AddressSanitizer and UBSan, on the CPU
only: tests/cpp/route_host_check.cpp (a stand-alone program with its own main)
is compiled together with xynet_amd/csrc/xyws_route.h, the source the kernel
and xyws_route_lookup share, and run over the routes and targets of
tests/route_cases.py, the table and each target in a heap buffer of its exact
size; then over a few thousand damaged tables, where only the clean exit
counts. The sanitizers are linked into the program itself; nothing is
preloaded and nothing here touches a GPU."""
import os
import struct
import subprocess

import route_cases as RC
import route_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAMAGED = 3000


def test_host_lookup_under_sanitizers(tmp_path):
    routes, targets = RC.TABLES["root"], [t for _, t in RC.TARGETS] + [b""]
    data = tmp_path / "inputs.bin"
    data.write_bytes(struct.pack("<I", len(routes)) +
                     b"".join(struct.pack("<I", len(k)) + k + struct.pack("<II", room, flags) for k, room, flags in routes) +
                     struct.pack("<I", len(targets)) + b"".join(struct.pack("<I", len(t)) + t for t in targets))
    exe = tmp_path / "route_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "xynet_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "route_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(data), str(DAMAGED)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    rows = [tuple(int(x) for x in line.split()) for line in lines[:-1]]
    assert len(rows) == 2 * len(targets)
    tab = M.table(routes)
    for s, t, status, room, route, key_off, key_len in rows:
        want = M.lookup(tab, targets[t])
        assert (status, room, route, key_off, key_len) == (
            want["status"], want["room"], want["route"], want["key_off"], want["key_len"]), (s, targets[t])
    assert lines[-1].startswith("damaged %d matched " % DAMAGED)
