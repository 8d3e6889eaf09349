"""The opt-in fp32 box rows of the fp16 plan (``hip_box_rows: fp32`` / ``FusedYoloV8(box_rows="fp32")`` / ``RVA_PLAN_BOX_F32``).

Contract held here:
  * the fp16 head tensor is still written in full and is bit-identical to the default plan's;
  * ``boxes32`` holds the fp32 value that was rounded into the fp16 row: ``boxes32.half()`` == rows 0-3, bit for bit;
  * nothing outside a level's anchor range is written in either tensor;
  * K2 in split mode never reads rows 0-3 of the head tensor (they are NaN in the K2 tests) and is otherwise the existing code:
    bit-exact against the oracle on the composite head (rows 0-3 from ``boxes32``, class rows = the fp16 rows widened);
  * the detector and ``PipelinedTicks`` hand K2 the side tensor of the head tensor's own slot.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops, synth
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig, config_from_dict
from realtime_video_analytics_32streams_amd.detector import HipYoloDetector, create_detector, filter_detections
from realtime_video_analytics_32streams_amd.engine import FusedYoloV8, module_order_convs
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
from realtime_video_analytics_32streams_amd.tracker import IouTracker
from realtime_video_analytics_32streams_amd.video_stream import FramePacket, SyntheticNv12Stream
from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density
from tests.helpers import plan_rounded_reference

pytestmark = pytest.mark.gpu

SENTINEL = -3.0
# |boxes32 - rounding-matched reference|: what assert_matches_rounded_reference grants on top of the store's rounding (summation
# order, fast exp / rcp).  The store's rounding is what the mode removes, so no half-ulp term here.
BOX_EPS = 0.03
# |boxes32 - plain fp32 module| on calibrated weights: twice the largest maximum recorded in profiles/box_rows_f32.json
# (n x 2: 0.0374, m x 4: 0.0370, s x 32: 0.0347 px -> 2 x 0.0374 = 0.075, rounded up to one significant digit).  The factor covers
# other kernel selections and seeds, whose summation order flips single fp16 roundings upstream.  Below 0.125 px, the half-ulp
# the fp16 rows carry between 256 and 512: the mode delivers.
FP32_MODULE_BOX_BOUND = 0.08


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t16):
    return t16.contiguous().view(torch.int16)


def _assert_side_tensor(got16, b32, want16, a0, n, what):
    """The three invariants of a head launch with a side tensor, on sentinel / NaN pre-filled tensors."""
    assert torch.equal(got16, want16), (what, "fp16 output differs from the existing entry point's")
    lv = b32[:, :, a0:a0 + n]
    assert torch.isfinite(lv).all(), what
    assert torch.equal(_bits(lv.half()), _bits(got16[:, :4, a0:a0 + n])), (what, "boxes32.half() != rows 0-3")
    outside = torch.ones_like(b32, dtype=torch.bool)
    outside[:, :, a0:a0 + n] = False
    assert torch.isnan(b32[outside]).all(), (what, "boxes32 written outside the level's anchor range")
    touched = torch.zeros_like(got16, dtype=torch.bool)
    touched[:, :, a0:a0 + n] = True
    assert torch.all(got16[~touched] == SENTINEL), (what, "head tensor written outside the level's anchor range")
    # the side tensor is the UNROUNDED value: most of its elements are not fp16 numbers
    assert float((lv.half().float() != lv).float().mean()) > 0.5, what


# ------------------------------------------------------------------------------------------------ head kernels
@pytest.mark.parametrize("Cin", [64, 128])
def test_fused_box_head_writes_the_side_tensor(Cin):
    """rva_conv1x1_head_box32_f16 (mode 1 of the fused head, variants 0 and 33-39): shapes of
    test_head_fused_conv_is_bit_identical_to_conv_then_head (ragged A, a0 != 0)."""
    B, H, W, nc = 3, 20, 13, 80
    A, a0, stride = H * W + 37, 21, 16.0
    g = torch.Generator().manual_seed(12)
    x = (torch.randn((B, H, W, Cin), generator=g) * 0.7).half().cuda()
    w = (torch.randn((64, Cin), generator=g) / Cin ** 0.5 * 2).half()
    b = torch.randn((64,), generator=g) * 0.3
    L, ctx = N.lib(), ops.context()
    s = _stream()
    wp = torch.zeros((64, 1, Cin), dtype=torch.float16); wp[:, 0] = w
    wp, bp = wp.cuda(), b.clone().cuda()
    for variant in [0] + list(range(33, 40)):
        want = torch.full((B, 4 + nc, A), SENTINEL, dtype=torch.float16, device="cuda")
        ctx.check(L.rva_conv1x1_head_f16(ctx.handle, C.c_void_p(x.data_ptr()), Cin, C.c_void_p(wp.data_ptr()), C.c_void_p(bp.data_ptr()),
                                         B, H, W, Cin, 64, 1, C.c_void_p(want.data_ptr()), nc, A, a0, C.c_float(stride), variant, s))
        got = torch.full((B, 4 + nc, A), SENTINEL, dtype=torch.float16, device="cuda")
        b32 = torch.full((B, 4, A), float("nan"), dtype=torch.float32, device="cuda")
        ctx.check(L.rva_conv1x1_head_box32_f16(ctx.handle, C.c_void_p(x.data_ptr()), Cin, C.c_void_p(wp.data_ptr()), C.c_void_p(bp.data_ptr()),
                                               B, H, W, Cin, C.c_void_p(got.data_ptr()), C.c_void_p(b32.data_ptr()), nc, A, a0,
                                               C.c_float(stride), variant, s), "rva_conv1x1_head_box32_f16")
        torch.cuda.synchronize()
        assert torch.all(want[:, 4:] == SENTINEL)                    # mode 1 writes the box rows only
        _assert_side_tensor(got, b32, want, a0, H * W, ("fused", Cin, variant))
    # a level that does not fit the anchor range, or no side tensor, is refused (bounds are checked before any launch)
    assert L.rva_conv1x1_head_box32_f16(ctx.handle, C.c_void_p(x.data_ptr()), Cin, C.c_void_p(wp.data_ptr()), C.c_void_p(bp.data_ptr()),
                                        B, H, W, Cin, C.c_void_p(got.data_ptr()), C.c_void_p(b32.data_ptr()), nc, A, A - H * W + 1,
                                        C.c_float(stride), 0, s) == N.RVA_ERR_ARG
    assert L.rva_conv1x1_head_box32_f16(ctx.handle, C.c_void_p(x.data_ptr()), Cin, C.c_void_p(wp.data_ptr()), C.c_void_p(bp.data_ptr()),
                                        B, H, W, Cin, C.c_void_p(got.data_ptr()), None, nc, A, a0, C.c_float(stride), 0, s) == N.RVA_ERR_ARG


def test_standalone_head_kernels_write_the_side_tensor():
    """rva_yolo_head_box32_f16 (one level, ragged A, a0 != 0) and rva_yolo_head3_box32_f16 (three levels in one launch)."""
    L, ctx = N.lib(), ops.context()
    s = _stream()
    B, nc = 3, 80
    g = torch.Generator().manual_seed(13)
    # one level
    H, W = 20, 13
    A, a0, stride = H * W + 37, 21, 16.0
    box = (torch.randn((B, H, W, 64), generator=g) * 2).half().cuda()
    cls = (torch.randn((B, H, W, nc), generator=g) * 2).half().cuda()
    want = torch.full((B, 4 + nc, A), SENTINEL, dtype=torch.float16, device="cuda")
    ctx.check(L.rva_yolo_head_f16(ctx.handle, C.c_void_p(box.data_ptr()), 64, C.c_void_p(cls.data_ptr()), nc, C.c_void_p(want.data_ptr()),
                                  B, H, W, nc, A, a0, C.c_float(stride), s))
    got = torch.full((B, 4 + nc, A), SENTINEL, dtype=torch.float16, device="cuda")
    b32 = torch.full((B, 4, A), float("nan"), dtype=torch.float32, device="cuda")
    ctx.check(L.rva_yolo_head_box32_f16(ctx.handle, C.c_void_p(box.data_ptr()), 64, C.c_void_p(cls.data_ptr()), nc, C.c_void_p(got.data_ptr()),
                                        C.c_void_p(b32.data_ptr()), B, H, W, nc, A, a0, C.c_float(stride), s), "rva_yolo_head_box32_f16")
    torch.cuda.synchronize()
    _assert_side_tensor(got, b32, want, a0, H * W, "head")
    assert L.rva_yolo_head_box32_f16(ctx.handle, C.c_void_p(box.data_ptr()), 64, C.c_void_p(cls.data_ptr()), nc, C.c_void_p(got.data_ptr()),
                                     C.c_void_p(b32.data_ptr()), B, H, W, nc, A, A - H * W + 1, C.c_float(stride), s) == N.RVA_ERR_ARG
    # three levels: block counts 2, 1, 1 with ragged tails (17 x 19 = 323, 9 x 10 = 90, 5 x 5 = 25 anchors)
    hs, ws, strides = [17, 9, 5], [19, 10, 5], [8.0, 16.0, 32.0]
    A3 = sum(h * w for h, w in zip(hs, ws))
    boxes = [(torch.randn((B, h, w, 64), generator=g) * 2).half().cuda() for h, w in zip(hs, ws)]
    clss = [(torch.randn((B, h, w, nc), generator=g) * 2).half().cuda() for h, w in zip(hs, ws)]
    bp, _k1 = N.ptr_array([t.data_ptr() for t in boxes])
    cp, _k2 = N.ptr_array([t.data_ptr() for t in clss])
    ldb, _k3 = N.i32_array([64] * 3)
    ldc, _k4 = N.i32_array([nc] * 3)
    hp, _k5 = N.i32_array(hs)
    wp, _k6 = N.i32_array(ws)
    sp = (C.c_float * 3)(*strides)
    # one image more than the batch in both tensors: the launch must leave it alone
    want3 = torch.full((B + 1, 4 + nc, A3), SENTINEL, dtype=torch.float16, device="cuda")
    ctx.check(L.rva_yolo_head3_f16(ctx.handle, bp, ldb, cp, ldc, C.c_void_p(want3.data_ptr()), B, hp, wp, nc, A3, sp, s))
    got3 = torch.full((B + 1, 4 + nc, A3), SENTINEL, dtype=torch.float16, device="cuda")
    b3 = torch.full((B + 1, 4, A3), float("nan"), dtype=torch.float32, device="cuda")
    ctx.check(L.rva_yolo_head3_box32_f16(ctx.handle, bp, ldb, cp, ldc, C.c_void_p(got3.data_ptr()), C.c_void_p(b3.data_ptr()), B, hp, wp, nc,
                                         A3, sp, s), "rva_yolo_head3_box32_f16")
    torch.cuda.synchronize()
    assert torch.equal(got3, want3) and torch.all(got3[B] == SENTINEL) and torch.isnan(b3[B]).all()
    assert torch.isfinite(b3[:B]).all() and torch.equal(_bits(b3[:B].half()), _bits(got3[:B, :4]))
    assert float((b3[:B].half().float() != b3[:B]).float().mean()) > 0.5


# ------------------------------------------------------------------------------------------------ split K2
def _split_case(seeds, negative_width_image=None, **gen):
    """Seeded [B, 84, 8400] heads as the split mode holds them: fp16 class rows, fp32 boxes that are NOT fp16 numbers.
    Returns (fp16 head with NaN in rows 0-3, boxes32, the composite fp32 head the oracle gets)."""
    heads = synth.make_head_batch(seeds, layout="CA", **gen)                 # float32 [B, 84, 8400]
    boxes = np.ascontiguousarray(heads[:, :4]).astype(np.float32)
    # push every box value off the fp16 grid (a quarter of an fp16 ulp): a kernel that read fp16 rows could not reproduce them
    ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(boxes), 2.0 ** -14))) - 10).astype(np.float32)
    boxes = (boxes.astype(np.float16).astype(np.float32) + 0.25 * ulp).astype(np.float32)
    if negative_width_image is not None:                                     # K3's irregular-box path: a candidate with w < 0
        b = negative_width_image
        score = heads[b, 5:].max(0) * heads[b, 4]
        boxes[b, 2, int(score.argmax())] *= -1.0
    assert np.all(boxes.astype(np.float16).astype(np.float32) != boxes)
    cls16 = heads[:, 4:].astype(np.float16)
    composite = np.concatenate([boxes, cls16.astype(np.float32)], 1)
    head16 = np.concatenate([np.full(boxes.shape, np.nan, np.float16), cls16], 1)
    return head16, boxes, composite


K2_CASES = {
    # name: (seeds, generator arguments, conf, iou, class filter, source size, image with a negative raw width)
    "1080p": ([300, 301, 302, 303], dict(n_obj=20), 0.25, 0.45, None, (1920, 1080), 2),
    "class-filter": ([310, 311, 312, 313], dict(n_obj=40), 0.25, 0.45, list(range(0, 79, 2)), (1920, 1080), None),
    "4k": ([320, 321, 322, 323], dict(n_obj=20), 0.3, 0.5, None, (3840, 2160), None),
    "identity": ([330, 331, 332, 333], dict(n_obj=20, content=(0, 0, 640, 640)), 0.25, 0.45, None, (640, 640), None),
    "busy": ([340, 341, 342, 343], dict(n_obj=150, dup=(8, 24)), 0.25, 0.6, None, (1920, 1080), None),
}


@pytest.mark.parametrize("head_dtype", [torch.float16, torch.float32], ids=["head-fp16", "head-fp32"])
@pytest.mark.parametrize("name", list(K2_CASES))
def test_split_k2_matches_the_oracle_on_the_composite_head(name, head_dtype):
    """rva_postprocess_boxes_batch against oracle.postprocess, bit-exact, with rows 0-3 of the head tensor filled with NaN."""
    seeds, gen, conf, iou, classes, wh, neg = K2_CASES[name]
    head16, boxes, composite = _split_case(seeds, neg, **gen)
    B, A = len(seeds), head16.shape[2]
    want = [orc.postprocess(composite[b], conf, iou, classes, wh) for b in range(B)]
    assert all(w["n"] >= 1 for w in want), [w["n"] for w in want]            # the oracle alone: no empty image
    if name == "busy":
        assert min(w["n_cand"] for w in want) > 1500
    raw = torch.from_numpy(head16).cuda().to(head_dtype).contiguous()
    assert torch.isnan(raw[:, :4]).all()
    ops.post_status(); ops.post_filter_stats()                                # clear what earlier tests left
    res = ops.postprocess(raw, conf, iou, classes, [N.letterbox(wh[0], wh[1], 640, 640)], max_det=A,
                          boxes=torch.from_numpy(boxes).cuda()).to_host()
    assert ops.post_status() == 0
    assert ops.post_filter_stats() == (B - 1 if neg is not None else B)       # the negative width took the unfiltered scan
    for b in range(B):
        got, w = res[b], want[b]
        assert got["n"] == w["n"] >= 1 and got["n_cand"] == w["n_cand"], (name, b)
        assert np.array_equal(got["anchor"], w["anchor"]) and np.array_equal(got["keep"], w["keep"]), (name, b)
        assert np.array_equal(got["cls"], w["cls"]) and np.array_equal(got["conf"], w["conf"]), (name, b)
        assert np.array_equal(got["boxes"], w["boxes"]) and np.isfinite(got["boxes"]).all(), (name, b)
    if classes:
        assert all(set(int(c) for c in r["cls"]) <= set(classes) for r in res)
    if neg is not None:
        assert composite[neg, 2].min() < 0


def test_split_k2_refuses_what_it_cannot_read():
    raw = torch.zeros((2, 84, 8400), dtype=torch.float16, device="cuda")
    m = [N.letterbox(1920, 1080, 640, 640)]
    with pytest.raises(ValueError, match="boxes"):
        ops.postprocess(raw, 0.25, 0.45, None, m, boxes=torch.zeros((2, 4, 8400), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match="boxes"):
        ops.postprocess(raw, 0.25, 0.45, None, m, boxes=torch.zeros((2, 4, 8399), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="boxes"):                             # [anchors, channels] heads have no split form
        ops.postprocess(raw.transpose(1, 2).contiguous(), 0.25, 0.45, None, m, boxes=torch.zeros((2, 4, 8400), device="cuda"))
    L, ctx = N.lib(), ops.context()
    out = ops.PostBuffers.allocate(2, 8400, raw.device)
    args = lambda ch, an: (ctx.handle, C.c_void_p(raw.data_ptr()), N.RVA_F16, C.c_void_p(raw.data_ptr()), 2, ch, an, 0.25, 0.45, None, 0,   # noqa: E731
                           (N.Letterbox * 1)(*m), 1, 8400, C.c_void_p(out.boxes.data_ptr()), C.c_void_p(out.scores.data_ptr()),
                           C.c_void_p(out.cls.data_ptr()), None, None, C.c_void_p(out.counts.data_ptr()), None, _stream())
    assert L.rva_postprocess_boxes_batch(*args(4, 8400)) == N.RVA_ERR_ARG      # channels < 5
    assert L.rva_postprocess_boxes_batch(*args(8400, 84)) == N.RVA_ERR_ARG     # [anchors, channels]
    assert b"rva_postprocess_boxes_batch" in L.rva_last_error(ctx.handle)


# ------------------------------------------------------------------------------------------------ plan
def _pair(net, batch, **kw):
    """The default plan and the split plan on the same weights with the same kernel selection."""
    p16 = FusedYoloV8(copy.deepcopy(net), batch, **kw)
    p32 = FusedYoloV8(copy.deepcopy(net), batch, autotune=False, box_rows="fp32")
    p32.copy_tuning(p16)
    assert p16.boxes32 is None and p32.boxes32 is not None and p32.boxes32.shape == (batch, 4, p32.A)
    assert [d for _, _, d in p16._tunable] == [d for _, _, d in p32._tunable] and p16._tuning_key() == p32._tuning_key()
    return p16, p32


@pytest.mark.parametrize("scale,batch", [("n", 2), ("s", 2), ("m", 4), ("s", 32)])
def test_split_plan_head_is_unchanged_and_boxes32_meets_box_eps(scale, batch):
    """The test that fails without the feature.  Head tensor bit-identical to the default plan's; boxes32 within BOX_EPS of the
    rounding-matched reference at EVERY element with no half-ulp allowance -- and the fp16 rows of the same run do not meet that
    bound (their maximum error exceeds 0.1 px; profiles/r04_fp16_error.json says 0.249)."""
    net = build_detector_net(scale, seed=0)
    p16, p32 = _pair(net, batch)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((batch, 3, 640, 640), device="cuda", generator=g).half()
    with torch.inference_mode():
        want16 = p16(x).clone()
        p32.out.fill_(SENTINEL); p32.boxes32.fill_(float("nan"))
        got16 = p32(x)
        b32 = p32.boxes32
        matched = torch.cat([plan_rounded_reference(net, x[i:i + 8]) for i in range(0, batch, 8)])[:, :4]
    torch.cuda.synchronize()
    assert torch.equal(got16, want16) and torch.isfinite(b32).all()
    assert torch.equal(_bits(b32.half()), _bits(got16[:, :4]))
    err32 = float((b32 - matched).abs().max())
    err16 = float((got16[:, :4].float() - matched).abs().max())
    print(f"box rows {scale} x {batch}: |boxes32 - matched| max {err32:.5f} px, |fp16 rows - matched| max {err16:.5f} px")
    assert err32 <= BOX_EPS, (scale, batch, err32)
    assert err16 > 0.1, (scale, batch, err16)                                   # the fp16 rows do not meet it: the test discriminates


@pytest.mark.parametrize("scale,batch", [("n", 2), ("m", 4), ("s", 32)])
def test_boxes32_against_the_plain_fp32_module_on_calibrated_weights(scale, batch):
    """|boxes32 - fp32 module| in input pixels on class-bias-calibrated weights (scores around 0.25, as _calibrated_error_report of
    tests/test_gpu_engine.py sets them up) within FP32_MODULE_BOX_BOUND -- what remains is the fp16 network itself (one rounding
    per layer, the box logits' included), not the store."""
    net = build_detector_net(scale, seed=0)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((batch, 3, 640, 640), device="cuda", generator=g).half()
    cal = copy.deepcopy(net).fuse().float().cuda()
    with torch.inference_mode():
        calibrate_detection_density(cal, x[:min(batch, 4)].float(), 0.25, 120)
        want = torch.cat([cal(x[i:i + 8].float()) for i in range(0, batch, 8)])
        p32 = FusedYoloV8(copy.deepcopy(cal), batch, box_rows="fp32")
        got16 = p32(x)
    torch.cuda.synchronize()
    assert int((want[:, 4:] >= 0.25).sum()) > 20 * batch                        # the scores matter
    err32 = float((p32.boxes32 - want[:, :4]).abs().max())
    err16 = float((got16[:, :4].float() - want[:, :4]).abs().max())
    print(f"box rows {scale} x {batch} vs fp32 module: boxes32 max {err32:.5f} px, fp16 rows max {err16:.5f} px")
    assert FP32_MODULE_BOX_BOUND < 0.125
    assert err32 <= FP32_MODULE_BOX_BOUND, (scale, batch, err32)


def test_boxes32_is_bit_identical_across_launch_modes_and_batch_position():
    net = build_detector_net("s", seed=0)
    B = 4
    p32 = FusedYoloV8(copy.deepcopy(net), B, box_rows="fp32")
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand((B, 3, 640, 640), device="cuda", generator=g).half()
    assert p32.fused_head_lanes()
    with torch.inference_mode():
        p32.concurrent_heads = False                                            # rva_yolov8_plan_run
        p32(x)
        torch.cuda.synchronize()
        run_h, run_b = p32.out.clone(), p32.boxes32.clone()
        p32.out.zero_(); p32.boxes32.zero_()
        p32.concurrent_heads = True                                             # rva_yolov8_plan_run_lanes
        p32(x)
        torch.cuda.synchronize()
        assert torch.equal(p32.out, run_h) and torch.equal(p32.boxes32.view(torch.int32), run_b.view(torch.int32))
        # a frame's position in the batch
        p32(torch.roll(x, 1, 0))
        torch.cuda.synchronize()
        assert torch.equal(torch.roll(p32.boxes32, -1, 0).view(torch.int32), run_b.view(torch.int32))
        assert torch.equal(torch.roll(p32.out, -1, 0), run_h)
        # a second output slot is one allocation of its own with its own side tensor
        h1 = p32.use_output(1)
        assert h1.data_ptr() != run_h.data_ptr() and p32.boxes32.data_ptr() != p32._boxes[0].data_ptr()
        assert p32.boxes32.data_ptr() - h1.data_ptr() == p32._out_layout[1] and p32._out_layout[1] % 256 == 0
        p32.boxes32.zero_()
        p32(x)
        torch.cuda.synchronize()
        assert torch.equal(p32.boxes32.view(torch.int32), run_b.view(torch.int32)) and torch.equal(p32.out, run_h)
        p32.use_output(0)
        # hipGraph replay of the pass
        p32.concurrent_heads = False
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            p32(x)
            torch.cuda.synchronize()
            with torch.cuda.graph(gr, stream=s):
                p32(x)
        p32.out.zero_(); p32.boxes32.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(p32.out, run_h) and torch.equal(p32.boxes32.view(torch.int32), run_b.view(torch.int32))


def test_box_flag_is_refused_on_an_fp32_plan():
    net = build_detector_net("n", seed=0).fuse()
    convs = module_order_convs(net)
    L, ctx = N.lib(), ops.context()
    keep, arr = [], (N.ConvWeights * len(convs))()
    for i, c in enumerate(convs):
        w = np.ascontiguousarray(c.weight.detach().float().numpy()); b = np.ascontiguousarray(c.bias.detach().float().numpy())
        keep += [w, b]
        arr[i].weight = w.ctypes.data_as(C.POINTER(C.c_float)); arr[i].bias = b.ctypes.data_as(C.POINTER(C.c_float))
        arr[i].cout, arr[i].cin, arr[i].k, arr[i].stride = w.shape[0], w.shape[1], w.shape[2], c.stride[0]
    d = N.YoloV8Desc(batch=1, height=640, width=640, depth_head=1, nc=80, reg_max=16, n_convs=len(convs),
                     flags=N.RVA_PLAN_F32 | N.RVA_PLAN_BOX_F32)
    d.widths[:] = [16, 32, 64, 128, 256]
    d.depth_backbone[:] = [1, 2, 2, 1]
    plan = C.c_void_p()
    assert L.rva_yolov8_plan_create(ctx.handle, C.byref(d), arr, C.byref(plan)) == N.RVA_ERR_ARG and not plan.value
    assert "RVA_PLAN_BOX_F32" in L.rva_last_error(ctx.handle).decode()
    with pytest.raises(ValueError, match="box_rows"):
        FusedYoloV8(build_detector_net("n", seed=0), 1, autotune=False, precision="fp32", box_rows="fp32")
    # the flag alone: the layout query reports the side tensor behind the fp16 head, and -1 without the flag
    for flags, want_off in ((N.RVA_PLAN_BOX_F32, (1 * 84 * 8400 * 2 + 255) // 256 * 256), (0, -1)):
        d.flags = flags
        ctx.check(L.rva_yolov8_plan_create(ctx.handle, C.byref(d), arr, C.byref(plan)), "rva_yolov8_plan_create")
        total, off = C.c_int64(), C.c_int64()
        ctx.check(L.rva_yolov8_plan_output_layout(plan, C.byref(total), C.byref(off)), "rva_yolov8_plan_output_layout")
        assert off.value == want_off and total.value == (want_off + 4 * 8400 * 4 if flags else 84 * 8400 * 2)
        L.rva_yolov8_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------ detector and pipeline
def _composite(res, b):
    """The fp32 head the oracle gets for image b of a split result: rows 0-3 from boxes32, class rows = the fp16 rows widened."""
    assert isinstance(res, ops.SplitHead) and res.head.dtype == torch.float16 and res.boxes.dtype == torch.float32
    return torch.cat([res.boxes[b], res.head[b, 4:].float()], 0).cpu().numpy()


def test_config0_shape_with_fp32_box_rows_matches_the_oracle():
    """BASELINE configs[0] in its own shape (one 640x360 host-BGR stream, YOLOv8n -- the head3 path --, batch 1) with ``half: true,
    hip_box_rows: fp32``: 10 ticks through predict -> filter_detections -> tracker.update == the oracle on the composite head."""
    cfg = config_from_dict({
        "max_concurrent_streams": 4, "stats_interval_seconds": 10,
        "streams": [{"name": "sim-1", "url": "/app/data/samples/demo.mp4", "enabled": True, "target_fps": 12, "batch_size": 1,
                     "warmup_seconds": 0.5, "reconnect_backoff": 2.0}],
        "detector": {"model_path": "/app/models/yolo/yolov8n.pt", "device": "cpu", "backend": "hip", "confidence_threshold": 0.35,
                     "iou_threshold": 0.5, "half": True, "warmup": False, "hip_box_rows": "fp32"},
        "tracker": {"type": "byte_track", "max_age": 30, "max_iou_distance": 0.5, "min_hits": 1}})
    stream = cfg.streams[0]
    det = create_detector(cfg.detector_for(stream))
    assert isinstance(det, HipYoloDetector) and det.engine == "fused" and det.box_rows == "fp32"
    frames = [synth.make_bgr(500 + t, 640, 360) for t in range(10)]
    sample = torch.from_numpy(np.stack([orc.preprocess_bgr(f, 640, 640, True)[0] for f in frames[:4]])).cuda()
    with torch.inference_mode():
        calibrate_detection_density(det.net, sample.contiguous(memory_format=torch.channels_last), cfg.detector.confidence_threshold, 40)
    det.invalidate_engine()
    raws = []
    infer = det._infer
    det._infer = lambda t: raws.append(infer(t)) or raws[-1]
    trk = IouTracker(cfg.tracker, max_streams=1, capacity=256)
    otr = orc.Tracker(1, cfg.tracker.max_age, cfg.tracker.max_iou_distance, cfg.tracker.min_hits)
    total, off_grid = 0, 0
    for t, frame in enumerate(frames):
        pkt = FramePacket(stream=stream, frame=frame, frame_id=t, timestamp=t / 12.0)
        dets = filter_detections(det.predict(pkt), cfg.detector.confidence_threshold)
        tracks = trk.update(stream.name, dets)
        assert not any(d.startswith("head1:") for _, _, d in det._plans[(1, 640, 640)]._tunable)       # YOLOv8n: k_head3 wrote the rows
        head = _composite(raws[t], 0)
        assert np.array_equal(raws[t].boxes[0].half().cpu().numpy().view(np.uint16), raws[t].head[0, :4].cpu().numpy().view(np.uint16))
        r = orc.postprocess(head, cfg.detector.confidence_threshold, cfg.detector.iou_threshold, None, (640, 360))
        keep = r["conf"].astype(np.float64) >= cfg.detector.confidence_threshold
        assert [d.class_id for d in dets] == [int(v) for v in r["cls"][keep]], t
        assert [d.confidence for d in dets] == [float(v) for v in r["conf"][keep]], t
        assert [list(d.bbox_xyxy) for d in dets] == [[float(x) for x in b] for b in r["boxes"][keep]], t
        w = otr.update(0, r["boxes"][keep].astype(np.float64), r["conf"][keep].astype(np.float64), r["cls"][keep].astype(np.int64))
        assert [x.track_id for x in tracks] == [int(v) for v in w["id"][:w["n"]]], t
        assert [list(x.bbox_xyxy) for x in tracks] == [[float(v) for v in b] for b in w["boxes"][:w["n"]]], t
        assert [(x.age, x.hits) for x in tracks] == [(int(a), int(h)) for a, h in zip(w["age"][:w["n"]], w["hits"][:w["n"]])], t
        # the fp16 rows would have given other boxes: the oracle on the plain fp16 head differs somewhere
        r16 = orc.postprocess(raws[t].head[0].float().cpu().numpy(), cfg.detector.confidence_threshold, cfg.detector.iou_threshold, None, (640, 360))
        off_grid += int(r16["n"] != r["n"] or not np.array_equal(r16["boxes"], r["boxes"]))
        total += len(dets)
    assert total > 0, "the calibrated detector produced nothing in 10 ticks"
    assert off_grid > 0, "boxes from boxes32 never differed from boxes from the fp16 rows"


def _run_32x1080p(depth, box_rows, net, T=12):
    """12 ticks of 32 x 1080p NV12 through PipelinedTicks with captured tails; per tick the tables and (split mode) the composite heads."""
    S = 32
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    det = HipYoloDetector(DetectorConfig(model_path="yolov8s.pt", backend="hip", model_type="yolov8", warmup=False, half=True,
                                         confidence_threshold=0.25, hip_box_rows=box_rows), net=copy.deepcopy(net))
    assert det.box_rows == box_rows
    tcfg = TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1)
    trk = IouTracker(tcfg, max_streams=S, capacity=1024)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth, use_graph=True)
    ticks = []

    def check(k):
        _, tables = runner.collect()
        par = k % runner.nslots
        if runner.net_streams >= 2:                                  # one plan per slot, output 0 of that plan
            plan, idx = det._plans[(S, 640, 640) if par == 0 else (S, 640, 640, par)], 0
        else:                                                        # one plan, one output per slot
            plan, idx = det._plans[(S, 640, 640)], par
        heads = None
        if box_rows == "fp32":
            res = ops.SplitHead(plan._outs[idx], plan._boxes[idx])
            assert plan._boxes[idx].data_ptr() - plan._outs[idx].data_ptr() == plan._out_layout[1]
            heads = [_composite(res, s) for s in range(S)]
        else:
            assert plan.boxes32 is None and not plan._boxes
        ticks.append(([orc.table_of(tables[s]) for s in range(S)], heads))
    done = 0
    for k in range(T):
        if k - done == runner.depth:
            check(done); done += 1
        runner.submit()
    while done < T:
        check(done); done += 1
    assert runner._captured
    return ticks, tcfg, det.config


@pytest.fixture(scope="module")
def calibrated_s_net():
    S = 8
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    net = build_detector_net("s", seed=0).fuse().half().cuda().to(memory_format=torch.channels_last)
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs], (640, 640), half=True)
        calibrate_detection_density(net, sample.contiguous(memory_format=torch.channels_last), 0.25, 120)
    return net


@pytest.fixture(scope="module")
def default_mode_tables(calibrated_s_net):
    """The same 12 ticks in the default mode (depth 4): what the split runs must differ from."""
    ticks, _, _ = _run_32x1080p(4, "fp16", calibrated_s_net)
    return [t[0] for t in ticks]


@pytest.mark.parametrize("depth", [1, 4])
def test_pipelined_ticks_hand_k2_the_side_tensor_of_the_slot(depth, calibrated_s_net, default_mode_tables):
    """32 x 1080p NV12, YOLOv8s, PipelinedTicks with captured tails: every tick's composite head through the oracle's post-process
    and one oracle tracker in canonical order gives the device's track tables (ids, age, hits, fp64 boxes) -- and those tables
    differ from the default mode's in at least one box coordinate (otherwise the side tensor is not reaching K2)."""
    S = 32
    ticks, tcfg, dcfg = _run_32x1080p(depth, "fp32", calibrated_s_net)
    otr = orc.Tracker(S, tcfg.max_age, tcfg.max_iou_distance, tcfg.min_hits)
    checked = 0
    for k, (tables, heads) in enumerate(ticks):
        for s in range(S):                                           # canonical order: tick-major, stream-minor
            r = orc.postprocess(heads[s], dcfg.confidence_threshold, dcfg.iou_threshold, None, (1920, 1080))
            m = r["conf"].astype(np.float64) >= dcfg.confidence_threshold
            want = otr.update(s, r["boxes"][m].astype(np.float64), r["conf"][m].astype(np.float64), r["cls"][m].astype(np.int64))
            assert tables[s] == orc.table_of(want), (k, s)
            checked += want["n"]
    assert checked > 20 * len(ticks)
    split_boxes = [row[5] for tables, _ in ticks for tab in tables for row in tab]
    default_boxes = [row[5] for tables in default_mode_tables for tab in tables for row in tab]
    assert split_boxes != default_boxes, "split-mode tables equal the default mode's: the side tensor is not reaching K2"


def test_default_detector_allocates_no_side_tensor_and_calls_the_existing_k2(monkeypatch):
    det = HipYoloDetector(DetectorConfig(model_path="yolov8n.pt", backend="hip", model_type="yolov8", warmup=False, half=True,
                                         confidence_threshold=0.25, hip_box_rows="fp16"), net=build_detector_net("n", seed=0))
    assert det.box_rows == "fp16"
    L = N.lib()
    calls = []
    real = L.rva_postprocess_batch

    def spy(*a):
        calls.append("rva_postprocess_batch")
        return real(*a)

    def never(*a):
        raise AssertionError("the default mode called rva_postprocess_boxes_batch")
    monkeypatch.setattr(L, "rva_postprocess_batch", spy)
    monkeypatch.setattr(L, "rva_postprocess_boxes_batch", never)
    stream = StreamConfig(name="cam", url="synthetic://640x360", warmup_seconds=0.0)
    with torch.inference_mode():
        raw = det._infer(torch.rand((2, 3, 640, 640), device="cuda").half())
    assert isinstance(raw, torch.Tensor) and not isinstance(raw, ops.SplitHead) and raw.dtype == torch.float16
    plan = det._plans[(2, 640, 640)]
    assert plan.box_rows == "fp16" and plan.boxes32 is None and plan._boxes == {} and plan.result() is plan.out
    assert plan.out.untyped_storage().nbytes() == 2 * 84 * 8400 * 2             # the head tensor alone
    det.predict(FramePacket(stream=stream, frame=synth.make_bgr(1, 640, 360), frame_id=0, timestamp=0.0))
    assert calls == ["rva_postprocess_batch"]
    # with half: false the key is accepted without effect, as it is behind an infer_fn
    d32 = HipYoloDetector(DetectorConfig(model_path="yolov8n.pt", backend="hip", model_type="yolov8", warmup=False, half=False,
                                         hip_box_rows="fp32"), net=build_detector_net("n", seed=0))
    assert d32.box_rows == "fp16" and d32.engine == "torch-fp32"
    dfn = HipYoloDetector(DetectorConfig(model_path="yolov8n.pt", backend="hip", model_type="yolov8", warmup=False, half=True,
                                         hip_box_rows="fp32"), infer_fn=lambda t: None)
    assert dfn.box_rows == "fp16"
