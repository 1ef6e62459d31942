"""The handshake grammar under AddressSanitizer and UBSan, on the CPU only:
tests/cpp/accept_host_check.cpp (a stand-alone program with its own main) is
compiled together with xynet_amd/csrc/xyws_accept.h, the source the kernel and
xyws_accept_request share, and run over the inputs of
tests/golden/handshake.json and all their truncations, each in a heap buffer of
its exact size. The sanitizers are linked into the program itself; nothing is
preloaded and nothing here touches a GPU."""
import os
import struct
import subprocess

import accept_cases as AC
import accept_model as M
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_grammar_under_sanitizers(tmp_path):
    inputs = [bytes.fromhex(e["req"]) for e in load_golden("handshake.json") if "req" in e]
    assert len(inputs) == len(AC.CASES)
    data = tmp_path / "inputs.bin"
    data.write_bytes(b"".join(struct.pack("<I", len(r)) + r for r in inputs))
    exe = tmp_path / "accept_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "xynet_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "accept_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == 2 * len(inputs)
    for i, policy, status, http, reason, consumed, resp_len, n_inc, n_acc, n_rej in rows:
        res, _ = M.accept(inputs[i], policy, max_request=M.MAX_REQUEST, out_cap=130)
        assert (status, http, reason, consumed, resp_len) == (
            res["status"], res["http_status"], res["reason"], res["consumed"], res["resp_len"]), (AC.NAMES[i], policy)
        assert n_inc + n_acc + n_rej == len(inputs[i]) + 1
        if AC.NAMES[i] in AC.TRUNCATED:
            cuts = [M.accept(inputs[i][:k], policy, max_request=M.MAX_REQUEST)[0]["status"]
                    for k in range(len(inputs[i]) + 1)]
            assert (n_inc, n_acc, n_rej) == (cuts.count(0), cuts.count(M.ACCEPTED), cuts.count(M.REJECTED))
