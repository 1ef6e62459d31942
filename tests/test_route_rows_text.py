"""xyws_route.hip moves its table rows through xynet_amd/csrc/xyws_rows.h like
the other sweep kernels: no word index and no layout assert of its own
(tests/test_rows_text.py's two checks applied to the new file), and the rows
the call adds pack and unpack as include/xyws.h lays them out
(tests/cpp/route_rows_host_check.cpp, a stand-alone program with its own main,
built with AddressSanitizer and UBSan linked into it and run on the CPU)."""
import os
import re
import subprocess

from test_rows_text import CSRC, code_of, layout_asserts, literal_subscripts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(CSRC, "xyws_route.hip")


def test_the_route_kernel_states_no_row_layout():
    assert literal_subscripts(PATH) == []
    assert layout_asserts(PATH) == []
    text = "\n".join(code_of(PATH))
    assert '#include "xyws_rows.h"' in text and '#include "xyws_route.h"' in text and '#include "xyws_lines.h"' in text
    # no row is addressed as words here at all: every access is a loader or a storer of xyws_rows.h
    assert not re.search(r"g_u64\s*\*", text)
    assert not re.search(r"\boffsetof\b|\bXYWS_WORD\b|\bXYWS_LD\b|\bXYWS_ST\b", text)
    # one launch, no atomics, and the 404 goes out through the shared line store
    assert len(re.findall(r"hipLaunchKernelGGL", text)) == 1 and "atomic" not in text and "put_line(" in text


def test_the_rows_header_states_the_route_rows():
    text = "\n".join(code_of(os.path.join(CSRC, "xyws_rows.h")))
    for pair in ("xyws_route_conn, rconn, reserved", "xyws_route_result, status, room",
                 "xyws_route_result, route, key_off"):
        assert "XYWS_ONE_WORD(%s)" % pair in text, pair
    assert "offsetof(xyws_roster_conn, room) / 4" in text
    assert literal_subscripts(os.path.join(CSRC, "xyws_rows.h")) == []


def test_route_row_layouts_under_sanitizers(tmp_path):
    exe = tmp_path / "route_rows_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "xynet_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "route_rows_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "0 failed"
