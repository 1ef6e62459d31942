"""xyws_inbox.hip moves its table rows through xynet_amd/csrc/xyws_rows.h like
the other sweep kernels: no word index and no layout assert of its own
(tests/test_rows_text.py's two checks applied to the new file), the call is the
five launches the header states, and the rows the call adds pack as
include/xyws.h lays them out (tests/cpp/inbox_rows_host_check.cpp, a
stand-alone program with its own main, built with AddressSanitizer and UBSan
linked into it and run on the CPU)."""
import os
import re
import subprocess

import xynet_amd._lib as L
from test_rows_text import CSRC, code_of, layout_asserts, literal_subscripts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(CSRC, "xyws_inbox.hip")


def test_the_inbox_kernels_state_no_row_layout():
    assert literal_subscripts(PATH) == []
    assert layout_asserts(PATH) == []
    text = "\n".join(code_of(PATH))
    assert '#include "xyws_rows.h"' in text and '#include "xyws_lines.h"' in text
    # no row is addressed as words here at all: every access is a loader or a storer of xyws_rows.h
    assert not re.search(r"g_u64\s*\*", text)
    assert not re.search(r"\boffsetof\b|\bXYWS_WORD\b|\bXYWS_LD\b|\bXYWS_ST\b", text)
    # every byte of a range goes out through the shared span copy, which ends its edge lines with put_line
    assert "copy_span(" in text and "store_line(" not in text and "store_edge(" not in text
    lines = "\n".join(code_of(os.path.join(CSRC, "xyws_lines.h")))
    assert "put_line(" in lines.split("void copy_span(")[1]


def test_the_call_is_five_launches_and_the_header_says_so():
    text = "\n".join(code_of(PATH))
    body = text.split("int xyws_inbox_streams(")[1].split("\n}\n")[0]
    assert len(re.findall(r"hipLaunchKernelGGL", text)) == 5 == len(re.findall(r"hipLaunchKernelGGL", body))
    assert not re.search(r"hipMemcpy|hipMemset|hipMalloc|hipStreamSynchronize|hipDeviceSynchronize|ctx->scratch", body)
    assert re.search(r"Five launches on `stream`", open(L.HEADER).read())
    # the only atomics are the order-free integer ones, and only the entry pass has them
    assert set(re.findall(r"\batomic\w+", text)) == {"atomicAdd", "atomicMax", "atomicOr"}
    entry_pass = text.split("k_inbox_entries(")[1].split("__global__")[0]
    assert len(re.findall(r"\batomic\w+\(", text)) == len(re.findall(r"\batomic\w+\(", entry_pass))
    assert not re.search(r"\bwhile\s*\(|__builtin_amdgcn_s_sleep", text)  # nothing spins
    # the copy pass's grid comes from m_cap alone
    assert re.search(r"fanout_grid\(m_cap,", body)


def test_the_rows_header_states_the_inbox_rows():
    text = "\n".join(code_of(os.path.join(CSRC, "xyws_rows.h")))
    for pair in ("xyws_inbox_entry, conn, flags", "xyws_inbox_carry, state, status", "xyws_inbox_conn, flags, reserved0",
                 "xyws_inbox_result, n_entries, status", "xyws_inbox_summary, n_conns, n_opened",
                 "xyws_inbox_summary, n_eof, n_broken", "xyws_inbox_summary, n_bad_entries, status"):
        assert "XYWS_ONE_WORD(%s)" % pair in text, pair
    assert literal_subscripts(os.path.join(CSRC, "xyws_rows.h")) == []


def test_inbox_row_layouts_under_sanitizers(tmp_path):
    exe = tmp_path / "inbox_rows_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "xynet_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "inbox_rows_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "0 failed"
