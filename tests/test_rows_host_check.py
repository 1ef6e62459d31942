"""The row layouts of the sweep kernels against include/xyws.h, on the CPU
only: tests/cpp/rows_host_check.cpp (a stand-alone program with its own main)
is compiled together with the pure part of xynet_amd/csrc/xyws_rows.h, the
header every sweep kernel reads and writes its table rows through, under
AddressSanitizer and UBSan, and run. It fails if a word index, a shift or a
mask of that header disagrees with the public structs. The sanitizers are
linked into the program itself; nothing is preloaded and nothing here touches
a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_layouts_under_sanitizers(tmp_path):
    exe = tmp_path / "rows_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "xynet_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "rows_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "0 failed"
