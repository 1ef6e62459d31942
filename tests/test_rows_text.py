"""The rows of the sweep tables are named in one place: the kernels of the
seven sweep calls and xyws_room.h move their table rows through
xynet_amd/csrc/xyws_rows.h and state no word index, and no layout assert, of
their own; xyws_rows.h spells its indices through offsetof. Text only: no
library, no GPU."""
import os
import re

import xynet_amd._lib as L

CSRC = os.path.join(L.PKG, "csrc")
DEVICE_FILES = ("xyws_streams.hip", "xyws_reply.hip", "xyws_reasm_streams.hip", "xyws_hold.hip", "xyws_broadcast.hip",
                "xyws_backlog.hip", "xyws_accept.hip", "xyws_room.h")
WORDS = r"(?:const\s+)?g_u64\s*\*"  # a pointer to a row's 64-bit words
DECL = re.compile(WORDS + r"\s*(?:const\s+)?(\w+)\s*[=;,)]")
CAST_SUBSCRIPT = re.compile(r"\(\(" + WORDS + r"\)[^\[\];]*\)\s*\[\s*\d+\s*\]")
ASSERT = re.compile(r"static_assert\s*\((.*?)\)\s*;", re.S)


def code_of(path):
    """The file's lines without // comments."""
    return [re.sub(r"//.*", "", line) for line in open(path).read().splitlines()]


def literal_subscripts(path):
    """Lines that subscript a row's words with an integer literal: [(line number, text)]."""
    lines = code_of(path)
    names = set(DECL.findall("\n".join(lines)))
    named = re.compile(r"\b(?:" + "|".join(sorted(names)) + r")\s*\[\s*\d+\s*\]") if names else None
    return [(n + 1, line.strip()) for n, line in enumerate(lines)
            if (named and named.search(line)) or CAST_SUBSCRIPT.search(line)]


def layout_asserts(path):
    """static_asserts over sizeof or offsetof of a public xyws_ struct."""
    return [a for a in ASSERT.findall("\n".join(code_of(path))) if re.search(r"\b(?:sizeof|offsetof)\s*\(\s*xyws_\w+", a)]


def violations(csrc=CSRC):
    """{file: what it states of a row's layout itself}, over the device files."""
    found = {}
    for name in DEVICE_FILES:
        path = os.path.join(csrc, name)
        bad = [f"line {n}: {text}" for n, text in literal_subscripts(path)]
        bad += ["static_assert: " + " ".join(a.split())[:80] for a in layout_asserts(path)]
        if bad:
            found[name] = bad
    return found


def test_the_kernels_state_no_row_layout():
    assert violations() == {}


def test_the_rows_header_spells_its_indices_through_offsetof():
    path = os.path.join(CSRC, "xyws_rows.h")
    assert literal_subscripts(path) == []
    text = "\n".join(code_of(path))
    assert re.search(r"#define XYWS_WORD\(T, f\) \(offsetof\(T, f\) / 8\)", text)
    assert re.search(r"#define XYWS_SHIFT\(T, f\) .*offsetof\(T, f\) % 8", text)
    # every device file reads its rows through it
    for name in DEVICE_FILES:
        assert '#include "xyws_rows.h"' in open(os.path.join(CSRC, name)).read(), name


def test_the_check_finds_what_it_forbids(tmp_path):
    (tmp_path / "k.hip").write_text(
        "const g_u64* const rq = (const g_u64*)(rows + i);\n"
        "uint64_t a = rq[2] >> 32;  // not rq[i]\n"
        "g_u64* res = out;\nres[lane] = 0;\nres[3] = 0;\n"
        "x = ((const g_u64*)(p + q))[0];\n"
        "static_assert(sizeof(xyws_room) == 32 &&\n   offsetof(xyws_room, wire) == 16, \"layouts\");\n"
        "static_assert(sizeof(s_w) == 8, \"own\");\n")
    path = str(tmp_path / "k.hip")
    assert [n for n, _ in literal_subscripts(path)] == [2, 5, 6]
    assert len(layout_asserts(path)) == 1
