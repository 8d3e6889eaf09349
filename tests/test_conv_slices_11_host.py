"""The YOLO11 slice layouts of tests/conv_slice_layouts.py without a GPU, as tests/test_conv_slices_v5_host.py does for YOLOv5:
the layout generators against (row stride, offset) triples worked out by hand from ``Builder::c2f`` with ``build_11``'s block
lambda, ``Builder::c3`` with ``k1 = 3``, ``Builder::c2psa`` and the class branch of ``Builder::build_11``; and the bound the GPU
test holds every kernel to (``helpers.assert_conv_close``) against the kernel restated in float32 -- it passes -- and against the
slice errors a kernel could make on these layouts -- each one fails it."""
import pytest

from tests import conv_slice_layouts as S
from tests.helpers import assert_conv_close

SHAPE1 = (3, 9, 7)                             # an M tail (189 pixels, tiles straddle images)


def _slices(lay):
    return (lay.cin, lay.cin_decl, lay.cout, lay.k, lay.inp, lay.out, lay.res, lay.res_own)


def test_c3k2_generator_against_hand_computed_slices():
    """YOLO11n `2` = C3k2(32, 64, n = 1, e = 0.25): c = 16, cat row 48, bottleneck 16 -> 8 -> 16.  `6` = C3k2(128, 128, n = 1,
    c3k): c = 64, outer row 192; the nested C3k(64, 64, 2) has c' = 32 and an inner row of 96."""
    b2 = S.N11_2
    assert list(b2) == ["cv1", "m0.cv1", "m0.cv2", "cv2"]
    assert _slices(b2["cv1"]) == (32, 32, 32, 1, (32, 0), (48, 0), None, False)
    assert _slices(b2["m0.cv1"]) == (16, 32, 8, 3, (48, 16), (8, 0), None, False)
    assert _slices(b2["m0.cv2"]) == (8, 32, 16, 3, (8, 0), (48, 32), (48, 16), False)           # shortcut and output both in cat
    assert _slices(b2["cv2"]) == (48, 64, 64, 1, (48, 0), (64, 0), None, False)
    assert all(lay.act == 1 and lay.stride == 1 and lay.live is None for lay in b2.values())
    b4, s4 = S.N11_4, S.S11_4
    assert _slices(b4["m0.cv1"]) == (32, 32, 16, 3, (96, 32), (16, 0), None, False)
    assert _slices(b4["m0.cv2"]) == (16, 32, 32, 3, (16, 0), (96, 64), (96, 32), False)
    assert _slices(s4["m0.cv1"]) == (64, 64, 32, 3, (192, 64), (32, 0), None, False)
    assert _slices(s4["m0.cv2"]) == (32, 32, 64, 3, (32, 0), (192, 128), (192, 64), False)
    b6 = S.N11_6
    assert list(b6) == ["cv1", "m0.cv1|cv2", "m0.m0.cv1", "m0.m0.cv2", "m0.m1.cv1", "m0.m1.cv2", "m0.cv3", "cv2"]
    assert _slices(b6["cv1"]) == (128, 128, 128, 1, (128, 0), (192, 0), None, False)
    assert _slices(b6["m0.cv1|cv2"]) == (64, 64, 64, 1, (192, 64), (96, 0), None, False)       # layout 5 of V11_STRIDE1_LAYOUTS
    assert _slices(b6["m0.m0.cv1"]) == (32, 32, 32, 3, (96, 0), (32, 0), None, False)          # row 6: 3x3 where YOLOv5 has 1x1
    assert _slices(b6["m0.m0.cv2"]) == (32, 32, 32, 3, (32, 0), (32, 0), (96, 0), True)        # shortcut in the inner row, own buffer out
    assert _slices(b6["m0.m1.cv1"]) == (32, 32, 32, 3, (32, 0), (32, 0), None, False)
    assert _slices(b6["m0.m1.cv2"]) == (32, 32, 32, 3, (32, 0), (96, 64), (32, 0), True)       # shortcut in m0's buffer, back into the row
    assert _slices(b6["m0.cv3"]) == (64, 64, 64, 1, (96, 32), (192, 128), None, False)         # row 7
    assert _slices(b6["cv2"]) == (192, 192, 128, 1, (192, 0), (128, 0), None, False)
    # the widest nested block, YOLO11m `4` = C3k2(256, 512, c3k, e = 0.25): c = 128, outer row 384, c' = 64
    assert _slices(S.M11_4["m0.cv1|cv2"]) == (128, 128, 128, 1, (384, 128), (192, 0), None, False)
    assert _slices(S.M11_4["m0.cv3"]) == (128, 128, 128, 1, (192, 64), (384, 256), None, False)
    # neck blocks: no residual anywhere
    for blk in (S.N11_16, S.N11_22):
        assert all(lay.res is None and not lay.res_own for lay in blk.values())
    assert _slices(S.N11_16["m0.cv2"]) == (16, 32, 32, 3, (16, 0), (96, 64), None, False)
    assert _slices(S.N11_22["m0.m1.cv2"]) == (64, 64, 64, 3, (64, 0), (192, 128), None, False)
    # the YOLOv5 output of the extended c3_layouts is what it was
    assert _slices(S.N_B4["m0.cv1"]) == (32, 32, 32, 1, (96, 0), (32, 0), None, False) and S.N_B4["m0.cv1"].name == "v5 n b4 c32 m0.cv1 of 2"
    assert _slices(S.N_B4["cv3"]) == (64, 64, 64, 1, (96, 32), (64, 0), None, False)


def test_c2psa_and_class_branch_generators_against_hand_computed_slices():
    """YOLO11n `10` = C2PSA(256, n = 1): c = 128, cv2's input row 256."""
    psa = S.N11_PSA
    assert list(psa) == ["cv1.a", "cv1.b", "m0.qkv", "m0.proj", "m0.ffn.0", "m0.ffn.1", "cv2"]
    acts = {key: lay.act for key, lay in psa.items()}
    assert acts == {"cv1.a": 1, "cv1.b": 1, "m0.qkv": 0, "m0.proj": 0, "m0.ffn.0": 1, "m0.ffn.1": 0, "cv2": 1}
    assert _slices(psa["cv1.a"]) == (256, 256, 128, 1, (256, 0), (256, 0), None, False)
    assert _slices(psa["cv1.b"]) == (256, 256, 128, 1, (256, 0), (128, 0), None, False)
    assert _slices(psa["m0.qkv"]) == (128, 128, 256, 1, (128, 0), (256, 0), None, False)
    assert _slices(psa["m0.proj"]) == (128, 128, 128, 1, (128, 0), (128, 0), (128, 0), True)            # row 10: ldr = ldo
    assert _slices(psa["m0.ffn.1"]) == (256, 256, 128, 1, (256, 0), (256, 128), (128, 0), True)         # row 11: ldr != ldo
    assert _slices(psa["cv2"]) == (256, 256, 256, 1, (256, 0), (256, 0), None, False)
    # two blocks: only the last ffn.1 writes cv2's input row
    assert _slices(S.L11_PSA["m0.ffn.1"]) == (256, 256, 128, 1, (256, 0), (128, 0), (128, 0), True)
    assert _slices(S.L11_PSA["m1.ffn.1"]) == _slices(psa["m0.ffn.1"])
    # class branch: nc 80 -> cc 80; nc 85 -> cr 85, cc 88; nc 200 on a 64-wide level -> min(nc, 100); level 4 of YOLO11n (ch 128, c3 64)
    cls, c85 = S.N11_CLS, S.N11_CLS85
    assert (_slices(cls["0.1"]), cls["0.1"].live) == ((64, 64, 80, 1, (64, 0), (80, 0), None, False), (64, 80))
    assert (_slices(cls["1.1"]), cls["1.1"].live) == ((80, 96, 80, 1, (80, 0), (80, 0), None, False), (80, 80))
    assert (_slices(c85["0.1"]), c85["0.1"].live) == ((64, 64, 88, 1, (64, 0), (88, 0), None, False), (64, 85))
    assert (_slices(c85["1.1"]), c85["1.1"].live) == ((88, 96, 88, 1, (88, 0), (88, 0), None, False), (85, 85))
    assert S.cls_branch_layouts(64, 200, "x")["1.1"].live == (100, 100) and S.cls_branch_layouts(64, 200, "x")["1.1"].cin == 104
    assert _slices(S.cls_branch_layouts(128, 80, "n l4", c3=64)["0.1"])[:3] == (128, 128, 80)


def test_invariants_of_the_yolo11_layouts():
    lays = S.V11_STRIDE1_LAYOUTS + S.V11_STRIDE2_LAYOUTS
    names = [lay.name for lay in lays]
    assert len(set(names)) == len(names) == 31
    assert not set(names) & {lay.name for lay in S.V5_STRIDE1_LAYOUTS + S.V5_STRIDE2_LAYOUTS}
    for lay in lays:
        for ld, off in (lay.inp, lay.out) + ((lay.res,) if lay.res else ()):
            assert ld % 8 == 0 and off % 8 == 0
        assert lay.inp[1] + lay.cin <= lay.inp[0] and lay.out[1] + lay.cout <= lay.out[0]
        assert lay.res is None or lay.res[1] + lay.cout <= lay.res[0]
        assert lay.cin_decl % 32 == 0 and 0 <= lay.cin_decl - lay.cin < 32
        # what a padded Cin reads past the last pixel's slice stays inside the row or the buffer's 64-byte slack
        assert max(lay.inp[1] + lay.cin_decl - lay.inp[0], 0) <= S.SLACK
        assert lay.live is None or (lay.live[0] <= lay.cin and lay.cin - lay.live[0] < 8 and lay.live[1] <= lay.cout and lay.cout - lay.live[1] < 8)
    # the 8-channel buffer: a row is 16 bytes, and the last pixel reads 24 of the 32 halves of slack
    lay = S.N11_2["m0.cv2"]
    assert lay.inp == (8, 0) and lay.inp[1] + lay.cin_decl - lay.inp[0] == 24


# number of the layout in V11_STRIDE1_LAYOUTS' comments -> (layout, the mutants that mean something on it).  The bound rejects every one of them on the
# operands make_case draws for every other test: none needed operands of its own
CASES = {
    "2 first conv 16->8": (S.N11_2["m0.cv1"], ("drop_last_8", "input_offset_ignored", "pad_columns_live")),
    "2 first conv 64->32": (S.S11_4["m0.cv1"], ("drop_last_8", "input_offset_ignored")),
    "3 second conv 8->16": (S.N11_2["m0.cv2"], ("drop_last_8", "pad_columns_live")),
    "3 second conv 16->32": (S.N11_4["m0.cv2"], ("drop_last_8", "pad_columns_live")),
    "4 closing cv2 48->64": (S.N11_2["cv2"], ("drop_last_8", "pad_columns_live")),
    "5 nested sibling": (S.N11_6["m0.cv1|cv2"], ("drop_last_8", "input_offset_ignored")),
    "6 nested m0.cv2": (S.N11_6["m0.m0.cv2"], ("ldr_is_ldo", "drop_last_8")),
    "6 nested m1.cv2": (S.N11_6["m0.m1.cv2"], ("ldr_is_ldo", "drop_last_8")),
    "7 nested cv3": (S.N11_6["m0.cv3"], ("drop_last_8", "input_offset_ignored")),
    "9 qkv": (S.N11_PSA["m0.qkv"], ("drop_last_8", "silu_despite_act0")),
    "10 proj": (S.N11_PSA["m0.proj"], ("drop_last_8", "silu_despite_act0")),
    "11 ffn.1": (S.N11_PSA["m0.ffn.1"], ("ldr_is_ldo", "drop_last_8", "silu_despite_act0")),
    "12 cls 64->88": (S.N11_CLS85["0.1"], ("drop_last_8",)),
    "12 cls 88->88": (S.N11_CLS85["1.1"], ("drop_last_8", "pad_columns_live")),
    "12 cls 80->80": (S.N11_CLS["1.1"], ("drop_last_8", "pad_columns_live")),
}


@pytest.mark.parametrize("key", list(CASES))
def test_bound_accepts_the_restatement_and_rejects_slice_mutants(key):
    lay, mutants = CASES[key]
    case = S.make_case(lay, SHAPE1)
    if lay.live is not None:                  # zero-extended as Builder::padded does: pad outputs are SiLU(0) = 0
        assert not bool(case["w"][:, lay.live[0]:].any()) and not bool(case["w"][lay.live[1]:].any())
        assert not bool(case["want"][:, lay.live[1]:].any())
    good = S.conv_slice_f32_cpu(lay, SHAPE1, case)
    assert good.shape == case["want"].shape
    assert_conv_close(good.double(), case["want"], case["res"], key)
    for mut in mutants:
        bad = S.conv_slice_f32_cpu(lay, SHAPE1, case, mut=mut)
        with pytest.raises(AssertionError):
            assert_conv_close(bad.double(), case["want"], case["res"], (key, mut))


def test_every_mutant_is_exercised():
    assert {m for _, muts in CASES.values() for m in muts} == set(S.MUTANTS)
    # each on the layouts where it means most
    assert "ldr_is_ldo" in CASES["11 ffn.1"][1]
    for key in ("3 second conv 8->16", "12 cls 88->88"):
        assert {"pad_columns_live", "drop_last_8"} <= set(CASES[key][1])
    for key in ("2 first conv 16->8", "5 nested sibling", "7 nested cv3"):
        assert "input_offset_ignored" in CASES[key][1]
    for key in ("9 qkv", "10 proj", "11 ffn.1"):
        assert "silu_despite_act0" in CASES[key][1]
