"""The scratch layout that host, kernels and Python share: stated once, in the
"scratch layout" section of xynet_amd/csrc/xyws_stream.h (one constant per
line, its value spelled out), and mirrored by name in xynet_amd/_lib.py. Every
mirrored constant equals the header's, the mirrored families are complete, no
two stats slots of one decoder share an index, and no other source file states
one of them again. Text only: no library, no GPU."""
import glob
import os
import re

import xynet_amd._lib as L

CSRC = os.path.join(L.PKG, "csrc")
HEADER = os.path.join(CSRC, "xyws_stream.h")
# families _lib.py mirrors whole, by the header's prefix
FAMILIES = ("ST_", "LT_", "R_", "DEC_", "DERR_")
POLICY_WORDS = ("POL_EPOCH", "POL_BYTES", "POL_FSMIN", "POL_FSMAX", "POL_DECODER", "POL_WORDS")
LINE = re.compile(r"^\s*(?:constexpr \w+ )?([A-Z][A-Z0-9_]*) = (0x[0-9a-fA-F]+|\d+)[,;]?\s*(?://.*)?$", re.M)


def header_constants():
    found = LINE.findall(open(HEADER).read())
    names = [n for n, _ in found]
    assert len(set(names)) == len(names), "a name is defined twice in xyws_stream.h"
    return {n: int(v, 0) for n, v in found}


def mirrored():
    """_lib.py's constants of the layout: {the header's name: value}."""
    mine = {k: v for k, v in vars(L).items() if k.startswith(FAMILIES) or k in POLICY_WORDS}
    mine["XYWS_NSTATS"] = L.NSTATS
    return mine


def test_the_header_states_the_layout():
    h = header_constants()
    for name in ("HEAD_TICKET", "HEAD_ERROR", "HEAD_TOTAL", "HEAD_EPOCH", "HEAD_CARRY", "HEAD_STATS", "HEAD_BYTES",
                 "HW_DONE", "HW_DPOL", "R_WORDS", "LW_DPOL", "LW_STAT", "XYWS_NSTATS") + POLICY_WORDS:
        assert name in h, f"{name} is not in the header's layout section"


def test_the_python_mirrors_are_the_headers():
    h, mine = header_constants(), mirrored()
    for name, v in mine.items():
        assert name in h, f"_lib.{name} has no {name} in xyws_stream.h"
        assert v == h[name], f"_lib.{name} = {v}, xyws_stream.h has {h[name]}"
    for name in h:
        if name.startswith(FAMILIES) or name in POLICY_WORDS:
            assert name in mine, f"{name} of xyws_stream.h has no mirror in _lib.py"


def test_stats_slots_of_one_decoder_are_distinct():
    h = header_constants()
    for prefix in ("ST_", "LT_"):
        owner = {}
        for name, v in h.items():
            if not name.startswith(prefix):
                continue
            assert v < h["XYWS_NSTATS"], f"{name} = {v} is outside the {h['XYWS_NSTATS']} stats words"
            assert v not in owner, f"{name} and {owner[v]} share slot {v}"
            owner[v] = name
        assert owner, f"no {prefix} slot found"


def test_the_layout_is_stated_once():
    h = header_constants()
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if path == HEADER:
            continue
        for name, _ in LINE.findall(open(path).read()):
            assert name not in h, f"{os.path.basename(path)} states {name} again"


def test_the_public_header_quotes_the_error_bits_right():
    h = header_constants()
    quoted = re.findall(r"\b(DERR_\w+) \((0x[0-9a-fA-F]+)\)", open(L.HEADER).read())
    assert quoted, "include/xyws.h names no DERR_ bit"
    for name, v in quoted:
        assert h.get(name) == int(v, 16), f"include/xyws.h says {name} ({v}), xyws_stream.h {h.get(name)}"
