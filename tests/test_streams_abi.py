"""CPU checks of xyws_decode_streams' boundary: the symbol is declared and
exported, xyws_conn keeps its layout, bad arguments are refused before any
device work, the kernel's geometry can be read without a device, and the C++
shim's wrapper compiles and links."""
import ctypes as C
import os
import subprocess

import xynet_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_and_exported():
    lib = L.load()
    assert "xyws_decode_streams" in L.declared_symbols()
    assert hasattr(lib, "xyws_decode_streams")
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"xyws_decode_streams", "xyws_debug_streams_geometry"} <= exported
    assert lib.xyws_abi_version() == 2  # (a function more breaks no caller)


def test_conn_layout_matches_header():
    assert C.sizeof(L.Conn) == 64
    off = {f[0]: getattr(L.Conn, f[0]).offset for f in L.Conn._fields_}
    assert (off["buf"], off["len"], off["carry"], off["frames"], off["cap"]) == (0, 8, 16, 24, 32)
    assert off["reserved"] == 40
    src = open(L.HEADER).read()
    body = src[src.index("typedef struct xyws_conn {"):src.index("} xyws_conn;")]
    names = [ln.split(";")[0].split()[-1].split("[")[0] for ln in body.splitlines()[1:] if ";" in ln]
    assert names == [f[0] for f in L.Conn._fields_]


def test_bad_arguments_are_refused_without_a_device():
    lib = L.load()
    assert lib.xyws_decode_streams(None, None, 0, None, 0, None) == -1
    table = (L.Conn * 2)()
    assert lib.xyws_decode_streams(None, table, 2, None, 0, None) == -1
    assert lib.xyws_debug_streams_geometry(None) == -1


def test_geometry_without_a_device():
    lib = L.load()
    out = (C.c_uint64 * 4)()
    assert lib.xyws_debug_streams_geometry(out) == 0
    window, lanes, per_wg, grid_cap = out
    assert window % 16 == 0 and window >= 64
    assert lanes % 64 == 0 and lanes >= 64
    assert per_wg >= 1 and per_wg * lanes <= 1024
    assert 1 <= grid_cap <= 1 << 20


SHIM_PROG = r"""
#include <cstdio>
#include "xyws/websocket.hpp"
static_assert(sizeof(xyws_conn) == 64);
static_assert(offsetof(xyws_conn, carry) == 16 && offsetof(xyws_conn, cap) == 32);
int main() {
  try {
    xyws::context ctx(0);
    xyws::decode_streams(ctx, nullptr, 0, nullptr, 0, nullptr);  // n == 0: nothing is launched
    std::puts("device");
  } catch (const xyws::error& e) {
    std::printf("error %d\n", e.code());
  }
  // the C entry point refuses a null context whatever else it is given
  xyws_conn table[1] = {};
  std::printf("null %d\n", xyws_decode_streams(nullptr, table, 1, nullptr, 0, nullptr));
  return 0;
}
"""


def test_cpp_shim_names_decode_streams(tmp_path):
    src = tmp_path / "streams.cpp"
    src.write_text(SHIM_PROG)
    exe = tmp_path / "streams"
    libdir = os.path.dirname(L.lib_path())
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe), "-L", libdir, "-lxyws", f"-Wl,-rpath,{libdir}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    lines = out.stdout.split("\n")
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    assert lines[0] == ("device" if has_gpu else "error -2")
    assert lines[1] == "null -1"
