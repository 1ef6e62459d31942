"""CPU checks of XYWS_DFO_DYNAMIC at xyws_deflate_streams' boundary: the option bit and every other bit of opts, the
result word it fills, and the code builder's debug entry, every refusal decided on the arguments alone (no device)."""
import ctypes as C

import pytest

import xynet_amd._lib as L


@pytest.mark.parametrize("opts, want", [(2, 0), (0, 0), (1, -1), (3, -1), (4, -1), (0x80000002, -1)])
def test_the_option_bit(opts, want):
    p = C.cast(C.create_string_buffer(4096), C.c_void_p)
    assert L.DFO_DYNAMIC == 2
    assert [L.load().xyws_deflate_streams(c, p, p, p, p, 0, opts, p, p, p, p, None) for c in (p, None)] == [want, -1]


def test_n_dynamic_reads_offset_28():
    row = L.DeflateResult.from_buffer_copy(bytes(28) + (7).to_bytes(4, "little"))
    assert row.n_dynamic == 7 and L.DeflateResult.reserved0.offset == 28
    with pytest.raises(AttributeError):
        row.n_dynamic = 1


def test_the_builder_entry_refuses_without_a_device():
    p = C.cast(C.create_string_buffer(4096), C.c_void_p)
    call = L.load().xyws_debug_deflate_code_lengths
    assert "xyws_debug_deflate_code_lengths" not in L.declared_symbols()
    for ctx, freq, nsym, limit, lens in ((None, p, 19, 7, p), (p, None, 19, 7, p), (p, p, 19, 7, None), (p, p, 0, 7, p),
                                         (p, p, 287, 15, p), (p, p, 19, 0, p), (p, p, 19, 16, p)):
        assert call(ctx, freq, nsym, limit, lens, None) == -1
