"""Host side of the fp16 plan's row windows: ``rva_conv_rows_through`` (include/rva.h) -- which output rows of a convolution see
a given window of input rows -- against a brute-force receptive-field computation, and the windows it yields when chained
through the early layers of a 640-row plan whose content rows are [140, 500) (a 1080p frame letterboxed to 640 x 360)."""
import ctypes as C

import numpy as np
import pytest

from realtime_video_analytics_32streams_amd import _native as N


def rows_through(k, stride, h_in, lo, hi):
    a, b = C.c_int32(-1), C.c_int32(-1)
    rc = N.lib().rva_conv_rows_through(k, stride, h_in, lo, hi, C.byref(a), C.byref(b))
    assert rc == N.RVA_OK, (k, stride, h_in, lo, hi, rc)
    return int(a.value), int(b.value)


def brute_rows(k, stride, h_in, lo, hi):
    """Output rows whose taps (pad k // 2; rows outside the image are zero padding, never dependent) meet input rows [lo, hi)."""
    pad = k // 2
    h_out = (h_in + 2 * pad - k) // stride + 1
    dep = np.zeros(h_in, dtype=bool)
    dep[lo:hi] = True
    out = np.zeros(h_out, dtype=bool)
    for o in range(h_out):
        for t in range(k):
            i = o * stride - pad + t
            if 0 <= i < h_in and dep[i]:
                out[o] = True
    return out


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("h_in", [7, 8, 20, 21, 160])
def test_rows_through_matches_the_receptive_field(k, stride, h_in):
    for lo in range(h_in):
        for hi in range(lo + 1, h_in + 1):
            want = brute_rows(k, stride, h_in, lo, hi)
            a, b = rows_through(k, stride, h_in, lo, hi)
            got = np.zeros_like(want)
            assert 0 <= a <= b <= len(want), (lo, hi, a, b)
            got[a:b] = True
            # the dependent rows of a contiguous input window are contiguous: the half-open window is exactly that set
            assert np.array_equal(got, want), (k, stride, h_in, lo, hi, (a, b), np.flatnonzero(want))


def test_rows_through_rejects_bad_windows():
    a, b = C.c_int32(), C.c_int32()
    f = N.lib().rva_conv_rows_through
    for args in [(3, 1, 8, 3, 3), (3, 1, 8, 5, 4), (3, 1, 8, -1, 4), (3, 1, 8, 0, 9), (2, 1, 8, 0, 8), (3, 3, 8, 0, 8), (3, 1, 0, 0, 1)]:
        assert f(*args, C.byref(a), C.byref(b)) == N.RVA_ERR_ARG, args


def test_chained_windows_of_a_letterboxed_1080p_frame():
    """The table of the design notes: 640 rows, content rows [140, 500), through the 3x3 pad-1 geometry of YOLOv8s's backbone."""
    w = (140, 500)
    w = rows_through(3, 2, 640, *w)
    assert w == (70, 251)                              # stem, inside the fused launch
    w = rows_through(3, 2, 320, *w)
    assert w == (35, 126)                              # b1 = the fused launch's output
    b1 = w
    assert rows_through(1, 1, 160, *b1) == (35, 126)   # b2.cv1
    w = rows_through(3, 1, 160, *b1)
    assert w == (34, 127)
    w = rows_through(3, 1, 160, *w)
    assert w == (33, 128)                              # b2's bottleneck; b2.cv2 takes the union of its inputs: the same
    w = rows_through(3, 2, 160, *w)
    assert w == (16, 65)                               # b3, b4.cv1
    got = []
    for _ in range(4):
        w = rows_through(3, 1, 80, *w)
        got.append(w)
    assert got == [(15, 66), (14, 67), (13, 68), (12, 69)]      # b4's four 3x3; b4.cv2: (12, 69)
    w = rows_through(3, 2, 80, *w)
    assert w == (6, 35)                                # b5, b6.cv1
    got = []
    for _ in range(4):
        w = rows_through(3, 1, 40, *w)
        got.append(w)
    assert got == [(5, 36), (4, 37), (3, 38), (2, 39)]          # b6's four 3x3; b6.cv2: (2, 39)
    w = rows_through(3, 2, 40, *w)
    assert w == (1, 20)                                # b7
    w = rows_through(3, 1, 20, *w)
    w = rows_through(3, 1, 20, *w)
    assert w == (0, 20)                                # from b8's bottleneck on every row depends on the content
