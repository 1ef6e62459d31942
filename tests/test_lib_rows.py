"""The row helpers of xynet_amd/_lib.py on the CPU: alloc_rows and row_ptr size
and address a table by its ctypes structure, and a Table filled through its
fields reads back through read_rows, for every row structure and for 0, 1 and
3 rows."""
import ctypes as C

import pytest
import torch

from xynet_amd import _lib

# every structure of _lib but xyws_arena_result, which is a host result with a pointer into it, never a table row
STRUCTS = sorted((s for s in vars(_lib).values()
                  if isinstance(s, type) and issubclass(s, C.Structure) and s not in (C.Structure, _lib.ArenaResult)),
                 key=lambda s: s.__name__)
COUNTS = (0, 1, 3)


def value(ftype, k, f, e=0):
    """A value other than zero for element e of field f of row k, within the field's width."""
    return (0x9E3779B97F4A7C15 * (k + 1) + 0x51 * (f + 1) + 0x1D * e) % ((1 << (8 * C.sizeof(ftype))) - 1) + 1


def fill(row, k):
    for f, (name, ftype) in enumerate(row._fields_):
        if issubclass(ftype, C.Array):
            setattr(row, name, ftype(*[value(ftype._type_, k, f, e) for e in range(ftype._length_)]))
        else:
            setattr(row, name, value(ftype, k, f))


def fields(row):
    return [list(v) if isinstance(v, C.Array) else v for v in (getattr(row, name) for name, _ in row._fields_)]


def test_the_structures_are_found():
    assert len(STRUCTS) >= 40 and _lib.Conn in STRUCTS and _lib.BacklogCarry in STRUCTS and _lib.Message in STRUCTS


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("struct", STRUCTS, ids=lambda s: s.__name__)
def test_alloc_rows_and_row_ptr(struct, n):
    size = C.sizeof(struct)
    t = _lib.alloc_rows(struct, n, "cpu")
    assert t.dtype == torch.uint8 and t.numel() == max(n, 1) * size
    assert not bool(t.any())
    assert _lib.alloc_rows(struct, n, "cpu", zero=False).numel() == max(n, 1) * size
    per = _lib.alloc_rows(struct, n, "cpu", per=5)
    assert per.numel() == max(n, 1) * 5 * size and not bool(per.any())
    for k in range(max(n, 1) + 1):
        assert _lib.row_ptr(t, struct, k) == t.data_ptr() + k * size
    assert _lib.row_ptr(t, struct) == t.data_ptr()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("struct", STRUCTS, ids=lambda s: s.__name__)
def test_a_table_reads_back_field_for_field(struct, n):
    """(The last-row read needs a row: n = 0 only checks that nothing is read.)"""
    tab = _lib.Table(struct, n)
    for k in range(n):
        fill(tab[k], k)
    t = tab.upload("cpu")
    assert t.numel() == max(n, 1) * C.sizeof(struct)
    rows = _lib.read_rows(struct, t, n)
    assert len(rows) == n
    for k, row in enumerate(rows):
        assert fields(row) == fields(tab[k])
        assert any(fields(row))
    if n:
        last = _lib.read_rows(struct, t, 1, first=n - 1)
        assert len(last) == 1 and fields(last[0]) == fields(tab[n - 1])
