"""xyws_outbox.hip moves its table rows through xynet_amd/csrc/xyws_rows.h like
the other sweep kernels: no word index and no layout assert of its own
(tests/test_rows_text.py's two checks applied to the new file), and the rows
the call adds pack as include/xyws.h lays them out
(tests/cpp/outbox_rows_host_check.cpp, a stand-alone program with its own main,
built with AddressSanitizer and UBSan linked into it and run on the CPU)."""
import os
import re
import subprocess

from test_rows_text import CSRC, code_of, layout_asserts, literal_subscripts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(CSRC, "xyws_outbox.hip")


def test_the_outbox_kernels_state_no_row_layout():
    assert literal_subscripts(PATH) == []
    assert layout_asserts(PATH) == []
    text = "\n".join(code_of(PATH))
    assert '#include "xyws_rows.h"' in text and '#include "xyws_lines.h"' in text
    # no row is addressed as words here at all: every access is a loader or a storer of xyws_rows.h
    assert not re.search(r"g_u64\s*\*", text)
    assert not re.search(r"\boffsetof\b|\bXYWS_WORD\b|\bXYWS_LD\b|\bXYWS_ST\b", text)
    # three launches, no atomics, and every byte of the pack goes out through the shared whole-line store
    assert len(re.findall(r"hipLaunchKernelGGL", text)) == 3 and "atomic" not in text
    assert "store_line(" in text and "load_bytes(" in text and "low_bytes(" in text
    assert "store_edge(" not in text and "put_line(" not in text


def test_the_rows_header_states_the_outbox_rows():
    text = "\n".join(code_of(os.path.join(CSRC, "xyws_rows.h")))
    for pair in ("xyws_outbox_entry, conn, flags", "xyws_outbox_summary, n_close, n_truncated",
                 "xyws_outbox_summary, n_deferred, status"):
        assert "XYWS_ONE_WORD(%s)" % pair in text, pair
    assert literal_subscripts(os.path.join(CSRC, "xyws_rows.h")) == []


def test_outbox_row_layouts_under_sanitizers(tmp_path):
    exe = tmp_path / "outbox_rows_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "xynet_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "outbox_rows_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "0 failed"
