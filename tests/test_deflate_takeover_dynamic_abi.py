"""XYWS_DFO_WINDOW_DYNAMIC at the boundary, on the CPU (n == 0, no device): the windows call takes that bit and no other, the sibling refuses it."""
import ctypes as C

import pytest

import xynet_amd._lib as L


@pytest.mark.parametrize("opts", [0, 4, 1, 2, 3, 5, 6, 8, 0x80000004])
def test_the_bit_is_the_windows_call_s_alone(opts):
    P, lib = C.cast(C.create_string_buffer(4096), C.c_void_p), L.load()
    assert L.DFO_WINDOW_DYNAMIC == 4 and L.DFO_DYNAMIC == 2
    assert lib.xyws_deflate_windows_streams(P, P, P, P, P, 0, P, P, None, 1, opts, P, P, P, None, P, None) == (0 if opts in (0, 4) else -1)
    assert lib.xyws_deflate_streams(P, P, P, P, P, 0, opts, P, P, P, P, None) == (0 if opts in (0, 2) else -1)
