"""The YOLOv5 slice layouts of tests/conv_slice_layouts.py without a GPU: the layout generator against (row stride, offset)
triples worked out by hand from ``Builder::c3``, and the bound the GPU test holds every kernel to (``helpers.assert_conv_close``)
against the kernel restated in float32 -- it passes -- and against the slice errors a kernel could make on these layouts -- each
one fails it.  A bound that a wrong row stride or a live padding column slipped through would make the GPU test worthless."""
import pytest

from tests import conv_slice_layouts as S
from tests.helpers import assert_conv_close

SHAPE1, SHAPE2 = (3, 9, 7), (2, 12, 20)        # an M tail (189 pixels, tiles straddle images); stride 2 on even sizes


def test_layout_generator_against_hand_computed_slices():
    """YOLOv5n b2 = C3(32, 32, n = 1): c = 16, cat row 48.  b4 = C3(64, 64, n = 2): c = 32, cat row 96."""
    def slices(lay):
        return (lay.cin, lay.cin_decl, lay.cout, lay.k, lay.inp, lay.out, lay.res, lay.res_own)
    b2 = S.N_B2
    assert list(b2) == ["cv1|cv2", "m0.cv1", "m0.cv2", "cv3"]
    assert slices(b2["cv1|cv2"]) == (32, 32, 32, 1, (32, 0), (48, 0), None, False)
    assert slices(b2["m0.cv1"]) == (16, 32, 16, 1, (48, 0), (16, 0), None, False)
    assert slices(b2["m0.cv2"]) == (16, 32, 16, 3, (16, 0), (48, 32), (48, 0), False)       # shortcut and output both in cat
    assert slices(b2["cv3"]) == (32, 32, 32, 1, (48, 16), (32, 0), None, False)
    b4 = S.N_B4
    assert list(b4) == ["cv1|cv2", "m0.cv1", "m0.cv2", "m1.cv1", "m1.cv2", "cv3"]
    assert slices(b4["cv1|cv2"]) == (64, 64, 64, 1, (64, 0), (96, 0), None, False)
    assert slices(b4["m0.cv1"]) == (32, 32, 32, 1, (96, 0), (32, 0), None, False)
    assert slices(b4["m0.cv2"]) == (32, 32, 32, 3, (32, 0), (32, 0), (96, 0), True)         # shortcut in cat, output a buffer of its own
    assert slices(b4["m1.cv1"]) == (32, 32, 32, 1, (32, 0), (32, 0), None, False)
    assert slices(b4["m1.cv2"]) == (32, 32, 32, 3, (32, 0), (96, 64), (32, 0), True)        # shortcut in m0's buffer, output in cat
    assert slices(b4["cv3"]) == (64, 64, 64, 1, (96, 32), (64, 0), None, False)
    # a neck block: no residual anywhere; the steps of build_v5
    assert all(lay.res is None and not lay.res_own for lay in S.N_H17.values())
    assert slices(S.N_H17["m0.cv2"]) == (32, 32, 32, 3, (32, 0), (96, 64), None, False)
    assert slices(S.h10_layout(128, 256, "n")) == (256, 256, 128, 1, (256, 0), (256, 128), None, False)
    assert slices(S.b1_layout(48, 96, "m"))[:6] == (48, 64, 96, 3, (48, 0), (96, 0)) and S.b1_layout(48, 96, "m").stride == 2
    names = [lay.name for lay in S.V5_STRIDE1_LAYOUTS + S.V5_STRIDE2_LAYOUTS]
    assert len(set(names)) == len(names) == 21
    for lay in S.V5_STRIDE1_LAYOUTS + S.V5_STRIDE2_LAYOUTS:
        for ld, off in (lay.inp, lay.out) + ((lay.res,) if lay.res else ()):
            assert ld % 8 == 0 and off % 8 == 0
        assert lay.inp[1] + lay.cin <= lay.inp[0] and lay.out[1] + lay.cout <= lay.out[0]
        assert lay.cin_decl % 32 == 0 and 0 <= lay.cin_decl - lay.cin < 32
        # what a padded Cin reads past the last pixel's slice stays inside the row or the buffer's 64-byte slack
        assert max(lay.inp[1] + lay.cin_decl - lay.inp[0], 0) <= S.SLACK


# layout number of the issue's table -> (layout, shape, the mutants that mean something on it)
CASES = {
    "2 cv1 c16": (S.N_B2["m0.cv1"], SHAPE1, ("drop_last_8", "pad_columns_live")),
    "2 cv1 c48": (S.M_B2["m0.cv1"], SHAPE1, ("drop_last_8", "pad_columns_live")),
    "3 first cv2 c16": (S.C16_N2["m0.cv2"], SHAPE1, ("ldr_is_ldo", "drop_last_8", "pad_columns_live")),
    "3 first cv2 c48": (S.M_B2["m0.cv2"], SHAPE1, ("ldr_is_ldo", "drop_last_8", "pad_columns_live")),
    "8 cv3 c16": (S.N_B2["cv3"], SHAPE1, ("drop_last_8", "input_offset_ignored")),
    "8 cv3 c48": (S.M_B2["cv3"], SHAPE1, ("drop_last_8", "input_offset_ignored")),
    "10 b1 n": (S.b1_layout(16, 32, "n"), SHAPE2, ("drop_last_8", "pad_columns_live")),
}


@pytest.mark.parametrize("key", list(CASES))
def test_bound_accepts_the_restatement_and_rejects_slice_mutants(key):
    lay, shape, mutants = CASES[key]
    case = S.make_case(lay, shape)
    good = S.conv_slice_f32_cpu(lay, shape, case)
    assert good.shape == case["want"].shape
    assert_conv_close(good.double(), case["want"], case["res"], key)
    for mut in mutants:
        bad = S.conv_slice_f32_cpu(lay, shape, case, mut=mut)
        with pytest.raises(AssertionError):
            assert_conv_close(bad.double(), case["want"], case["res"], (key, mut))


def test_every_mutant_is_exercised():
    # no convolution step of a YOLOv5 plan runs without activation: that mutant is planted on YOLO11's (test_conv_slices_11_host.py)
    assert {m for _, _, muts in CASES.values() for m in muts} == set(S.MUTANTS) - {"silu_despite_act0"}
