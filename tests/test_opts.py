"""The XYWS_OPT_* bits of a call's `opts` word: each stated once per language
(include/xyws.h and xynet_amd/csrc/xyws_stream.h in C, xynet_amd/_lib.py in
Python), every one a single bit, no two on the same bit, and the Python list
equal to the headers name by name. Text only: no library, no GPU."""
import os
import re

import xynet_amd._lib as L

HEADERS = (os.path.join(L.ROOT, "include", "xyws.h"), os.path.join(L.PKG, "csrc", "xyws_stream.h"))


def header_bits():
    found = []
    for h in HEADERS:
        found += re.findall(r"^#define XYWS_OPT_(\w+)\s+(0x[0-9a-fA-F]+)u\b", open(h).read(), re.M)
    return [(name, int(value, 16)) for name, value in found]


def test_each_option_is_one_bit_of_its_own():
    bits = header_bits()
    assert bits, "no XYWS_OPT_ define found"
    names = [n for n, _ in bits]
    assert len(set(names)) == len(names), "a name is defined twice"
    owner = {}
    for name, v in bits:
        assert 0 < v < 1 << 32 and v & (v - 1) == 0, f"XYWS_OPT_{name} = {v:#x} is not one bit of a uint32_t"
        assert v not in owner, f"XYWS_OPT_{name} and XYWS_OPT_{owner[v]} share {v:#x}"
        owner[v] = name


def test_the_python_list_is_the_headers():
    header = dict(header_bits())
    mine = {k[4:]: v for k, v in vars(L).items() if k.startswith("OPT_")}
    assert mine, "no OPT_ constant in _lib.py"
    for name, v in mine.items():
        assert name in header, f"_lib.OPT_{name} has no XYWS_OPT_{name}"
        assert v == header[name], f"_lib.OPT_{name} = {v:#x}, XYWS_OPT_{name} = {header[name]:#x}"
