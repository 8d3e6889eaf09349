"""Row windows of the fp16 plan (``rva_yolov8_plan_set_static_rows``, include/rva.h): the windowed launches of the convolution
primitives write exactly their rows, bit-identical to the whole launch; a plan told about a static border gives, once primed, the
output of a plan that never heard of it, bit for bit; and ``HipYoloDetector`` on letterboxed NV12 frames gives the head tensors of
a process in which ``RVA_PLAN_NO_STATIC_ROWS=1`` switches the windows off."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.engine import FusedYoloV8
from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SENTINEL = 0x7A5A           # fp16 bit pattern (51008.0): no convolution of the inputs below comes near it


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int16)


# ---------------------------------------------------------------------------------------------------
# Primitives
# ---------------------------------------------------------------------------------------------------
# B, H, W, Cin, Cout, k, stride, residual, (row stride, offset) of the input slice, of the output slice
CONV_SHAPES = {
    "1x1 64->64": (3, 21, 18, 64, 64, 1, 1, False, (64, 0), (64, 0)),
    "3x3 32->32": (2, 37, 50, 32, 32, 3, 1, False, (32, 0), (32, 0)),
    "3x3 64->64 residual": (2, 20, 24, 64, 64, 3, 1, True, (64, 0), (64, 0)),
    "3x3 s2 64->128": (2, 40, 24, 64, 128, 3, 2, False, (64, 0), (128, 0)),
    "1x1 96->64 slice": (2, 9, 7, 96, 64, 1, 1, False, (96 + 64, 32), (64 + 128, 128)),
}


def _windows(name, ho):
    w = [(0, ho), (0, 1), (ho - 1, ho), (ho // 2, ho // 2 + 1)]
    if "s2" in name:
        w.append((3, 11))                        # odd to odd
    return w


@pytest.mark.parametrize("name", list(CONV_SHAPES))
def test_windowed_conv_writes_its_rows_and_nothing_else(name):
    """Every variant that takes a row window, forced: rows [y0, y1) equal the whole launch bit for bit, every other row of the
    output slice and everything outside the slice keep the sentinel."""
    B, H, W, cin, cout, k, s, with_res, (ldi, offi), (ldo, offo) = CONV_SHAPES[name]
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((B * H * W, ldi), generator=g) * 0.5).half().cuda()
    w = (torch.randn((cout, k * k, cin), generator=g) / (cin * k * k) ** 0.5).half()
    L, ctx = N.lib(), ops.context()
    cpad = L.rva_conv_cout_pad(cout)
    wp = torch.zeros((cpad, k * k, cin), dtype=torch.float16)
    wp[:cout] = w
    bp = torch.zeros(cpad)
    bp[:cout] = torch.randn((cout,), generator=g) * 0.1
    wp, bp = wp.cuda(), bp.cuda()
    res = (torch.randn((B * Ho * Wo, cout), generator=g) * 0.5).half().cuda() if with_res else None
    blank = torch.full((B * Ho * Wo, ldo), SENTINEL, dtype=torch.int16, device="cuda")

    def launch(variant, out, y0, y1):
        return L.rva_conv2d_nhwc_f16_rows(ctx.handle, C.c_void_p(x.data_ptr() + 2 * offi), ldi, C.c_void_p(wp.data_ptr()),
                                          C.c_void_p(bp.data_ptr()), C.c_void_p(out.data_ptr() + 2 * offo), ldo,
                                          C.c_void_p(res.data_ptr()) if with_res else None, cout if with_res else 0, B, H, W, cin, cout,
                                          k, s, 1, variant, y0, y1, _stream())

    took_window = []
    for v in range(0, L.rva_conv_num_variants() + 1):
        full = blank.clone()
        rc = L.rva_conv2d_nhwc_f16_v(ctx.handle, C.c_void_p(x.data_ptr() + 2 * offi), ldi, C.c_void_p(wp.data_ptr()),
                                     C.c_void_p(bp.data_ptr()), C.c_void_p(full.data_ptr() + 2 * offo), ldo,
                                     C.c_void_p(res.data_ptr()) if with_res else None, cout if with_res else 0, B, H, W, cin, cout,
                                     k, s, 1, v, _stream())
        if rc == N.RVA_ERR_ARG:
            continue
        assert rc == N.RVA_OK, (v, rc)
        torch.cuda.synchronize()                 # a HIP error ends the test here: nothing more is launched after it
        full4 = full.reshape(B, Ho, Wo, ldo)
        assert not bool((full4[..., offo:offo + cout] == SENTINEL).all(dim=-1).any()), (v, "the whole launch left pixels unwritten")
        for (y0, y1) in _windows(name, Ho):
            out = blank.clone()
            rc = launch(v, out, y0, y1)
            if rc == N.RVA_ERR_ARG:
                assert (y0, y1) != (0, Ho), (v, "the whole image is a window every variant takes")
                continue
            assert rc == N.RVA_OK, (v, y0, y1, rc)
            torch.cuda.synchronize()
            want = blank.clone().reshape(B, Ho, Wo, ldo)
            want[:, y0:y1, :, offo:offo + cout] = full4[:, y0:y1, :, offo:offo + cout]
            assert torch.equal(out.reshape(B, Ho, Wo, ldo), want), (v, L.rva_conv_variant_name(v), y0, y1)
            if (y0, y1) != (0, Ho):
                took_window.append(v)
        # windows that are no windows
        for (y0, y1) in [(-1, 3), (2, 2), (3, 2), (0, Ho + 1)]:
            assert launch(v, blank.clone(), y0, y1) == N.RVA_ERR_ARG, (v, y0, y1)
    print(name, "variants that took a window:", sorted(set(took_window)))
    assert took_window, "no variant of this shape takes a row window"
    if cin % 64 == 0 and (k == 1 or s == 2):
        assert 0 in took_window                  # variant 0 picks the gather tile for these (Cin % 64 == 0) and passes the window on


@pytest.mark.parametrize("shape", [(2, 96, 160), (1, 64, 64)])
def test_windowed_stem2_writes_its_rows_and_nothing_else(shape):
    B, H, W = shape
    Ho, Wo = H // 4, W // 4
    g = torch.Generator().manual_seed(9)
    x = torch.rand((B, 3, H, W), generator=g).half().cuda()
    w1 = (torch.randn((64, 32), generator=g) * 0.2).half().cuda()
    b1 = (torch.randn((64,), generator=g) * 0.1).cuda()
    w2 = (torch.randn((64, 9, 32), generator=g) / 17.0).half().cuda()
    b2 = (torch.randn((64,), generator=g) * 0.1).cuda()
    L, ctx = N.lib(), ops.context()
    blank = torch.full((B, Ho, Wo, 64), SENTINEL, dtype=torch.int16, device="cuda")

    def launch(out, y0, y1):
        return L.rva_stem2_f16_rows(ctx.handle, C.c_void_p(x.data_ptr()), C.c_void_p(w1.data_ptr()), C.c_void_p(b1.data_ptr()),
                                    C.c_void_p(w2.data_ptr()), C.c_void_p(b2.data_ptr()), C.c_void_p(out.data_ptr()), 64, B, H, W, y0, y1, _stream())

    full = blank.clone()
    assert L.rva_stem2_f16(ctx.handle, C.c_void_p(x.data_ptr()), C.c_void_p(w1.data_ptr()), C.c_void_p(b1.data_ptr()), C.c_void_p(w2.data_ptr()),
                           C.c_void_p(b2.data_ptr()), C.c_void_p(full.data_ptr()), 64, B, H, W, _stream()) == N.RVA_OK
    torch.cuda.synchronize()
    assert not bool((full == SENTINEL).all(dim=-1).any())
    for (y0, y1) in [(0, 5), (7, 8), (3, Ho), (0, Ho)]:
        out = blank.clone()
        assert launch(out, y0, y1) == N.RVA_OK, (y0, y1)
        torch.cuda.synchronize()
        want = blank.clone()
        want[:, y0:y1] = full[:, y0:y1]
        assert torch.equal(out, want), (y0, y1)
    for (y0, y1) in [(-1, 3), (2, 2), (0, Ho + 1)]:
        assert launch(blank.clone(), y0, y1) == N.RVA_ERR_ARG, (y0, y1)


# ---------------------------------------------------------------------------------------------------
# Plans
# ---------------------------------------------------------------------------------------------------
def _dilate(dep):
    out = dep.copy()
    out[1:] |= dep[:-1]
    out[:-1] |= dep[1:]
    return out


def _down(dep):
    """3x3 stride 2 pad 1: output row o sees input rows 2o - 1, 2o, 2o + 1."""
    n = len(dep)
    return np.array([any(dep[i] for i in (2 * o - 1, 2 * o, 2 * o + 1) if 0 <= i < n) for o in range((n - 1) // 2 + 1)])


def _span(dep):
    idx = np.flatnonzero(dep)
    return (int(idx[0]), int(idx[-1]) + 1)


def _expected_backbone_rows(scale, H, top, bottom):
    """(step, window) of the backbone's first steps by brute force on sets of rows.  YOLOv8s: fused stem, and its 32-channel
    bottleneck is one launch (both 3x3); YOLOv8n: stem and b1 are steps of their own."""
    dep = np.zeros(H, dtype=bool)
    dep[top:bottom] = True
    out = []
    if scale == "s":
        dep = _down(_down(dep)); out.append(dep)                        # 0: stem + b1
        cv1 = dep; out.append(cv1)                                      # 1: b2.cv1
        dep = _dilate(_dilate(cv1)); out.append(dep)                    # 2: b2's bottleneck, one launch
        out.append(dep | cv1)                                           # 3: b2.cv2
        dep = _down(dep | cv1); out.append(dep)                         # 4: b3
    else:
        dep = _down(dep); out.append(dep)                               # 0: stem
        dep = _down(dep); out.append(dep)                               # 1: b1
        cv1 = dep; out.append(cv1)                                      # 2: b2.cv1
        dep = _dilate(cv1); out.append(dep)                             # 3
        dep = _dilate(dep); out.append(dep)                             # 4
        out.append(dep | cv1)                                           # 5: b2.cv2
        dep = _down(dep | cv1); out.append(dep)                         # 6: b3
    cv1 = dep; out.append(cv1)                                          # b4.cv1
    acc = cv1
    for i in range(4):                                                  # b4: two bottlenecks, four 3x3 (YOLOv8n: 32 channels, one launch each)
        dep = _dilate(dep)
        if scale == "s" or i % 2 == 1:
            out.append(dep)
        acc = acc | dep
    out.append(acc)                                                     # b4.cv2
    out.append(_down(acc))                                              # b5
    return [_span(d) for d in out], [len(d) for d in out]


WINDOWS = [(96, 160), (97, 161), (0, 100), (130, 256), (120, 124), (0, 256)]
PLANS = {"s": ("s", 3, (256, 64)), "n": ("n", 2, (256, 96))}
BORDER = 0.447


def _input(B, hw, top, bottom, seed, border=BORDER):
    x = torch.full((B, 3, *hw), border, dtype=torch.float16, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    x[:, :, top:bottom] = torch.rand((B, 3, bottom - top, hw[1]), device="cuda", generator=g).half()
    return x


@pytest.fixture(scope="module", params=list(PLANS))
def plan_pair(request):
    scale, B, hw = PLANS[request.param]
    saved = {k: os.environ.pop(k, None) for k in ("RVA_PLAN_NO_STATIC_ROWS", "RVA_PAIR32", "RVA_NO_STEM2", "RVA_NO_CIN_PAD", "RVA_TUNE_LAYER_OVERLAP")}
    try:
        net = build_detector_net(scale, seed=3)
        a = FusedYoloV8(net, B, hw=hw, autotune=False)
        b = FusedYoloV8(net, B, hw=hw, autotune=False)
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return scale, B, hw, net, a, b


@pytest.mark.parametrize("window", WINDOWS, ids=[f"{t}-{b}" for t, b in WINDOWS])
def test_windowed_plan_equals_the_plan_that_never_windows(plan_pair, window):
    scale, B, hw, net, a, b = plan_pair
    top, bottom = window
    b.set_static_rows(top, bottom)
    # the windows are what the receptive fields say, and the feature is on
    want, heights = _expected_backbone_rows(scale, hw[0], top, bottom)
    got = [b.step_rows(i) for i in range(len(want))]
    assert got == want, (got, want)
    if window != (0, hw[0]):
        assert any(w != (0, h) for w, h in zip(got[:3], heights[:3])), "the early steps' windows are the whole image"
        assert any(" r[" in d for _, _, d in b._tunable), "no tunable step's description carries its window"
    else:
        assert all(w == (0, h) for w, h in zip(got, heights)) and not any(" r[" in d for _, _, d in b._tunable)
    assert [a.step_rows(i) for i in range(len(want))] == [(0, h) for h in heights]

    # an unprimed plan's run_range covers all rows and does not prime: a second input with ANOTHER border still comes out right
    L = N.lib()
    for seed, border in ((1, BORDER), (2, 0.25)):
        x = _input(B, hw, top, bottom, seed, border)
        b.ctx.check(L.rva_yolov8_plan_run_range(b.handle, C.c_void_p(x.data_ptr()), C.c_void_p(b.out.data_ptr()), 0, b.n_launches, _stream()))
        got_rr = b.out.clone()
        assert torch.equal(_bits(got_rr), _bits(a(x))), ("run_range on an unprimed plan", border)

    b(_input(B, hw, top, bottom, 10))                      # prime: one complete run on this border
    for seed in (11, 12, 13):
        x = _input(B, hw, top, bottom, seed)
        assert torch.equal(_bits(b(x)), _bits(a(x))), (window, seed)
        if seed == 12:
            # another kernel on a windowed step: the plan covers all rows once more, then windows again
            idx = next((i for i, (_, _, d) in enumerate(b._tunable) if " r[" in d), 0)
            for v in (36, 2):                              # a gather tile that takes windows, a kernel that does not
                if b._tunable[idx][0](_stream(), v) == N.RVA_OK:
                    b._tunable[idx][1]["variant"] = v
                    a._tunable[idx][1]["variant"] = v      # the same kernel in the reference plan: bit-equality is per kernel
                    for s2 in (20, 21):
                        x2 = _input(B, hw, top, bottom, s2)
                        assert torch.equal(_bits(b(x2)), _bits(a(x2))), (window, "after set_variant", v, s2)
            b._tunable[idx][1]["variant"] = 0
            a._tunable[idx][1]["variant"] = 0
    torch.cuda.synchronize()


def test_windowed_plan_with_fp32_box_rows():
    scale, B, hw = PLANS["s"]
    net = build_detector_net(scale, seed=3)
    a = FusedYoloV8(net, B, hw=hw, autotune=False, box_rows="fp32")
    b = FusedYoloV8(net, B, hw=hw, autotune=False, box_rows="fp32", static_rows=(96, 160))
    assert b.step_rows(0) != a.step_rows(0)
    b(_input(B, hw, 96, 160, 30))
    for seed in (31, 32, 33):
        x = _input(B, hw, 96, 160, seed)
        a(x), b(x)
        assert torch.equal(_bits(a.out), _bits(b.out)) and torch.equal(a.boxes32.view(torch.int32), b.boxes32.view(torch.int32)), seed


def test_static_rows_arguments_and_fp32_plans():
    scale, B, hw = PLANS["n"]
    net = build_detector_net(scale, seed=3)
    p = FusedYoloV8(net, B, hw=hw, autotune=False)
    L = N.lib()
    for top, bottom in [(-1, 10), (10, 10), (20, 10), (0, hw[0] + 1)]:
        assert L.rva_yolov8_plan_set_static_rows(p.handle, top, bottom) == N.RVA_ERR_ARG
    f = FusedYoloV8(net, B, hw=hw, autotune=False, precision="fp32")
    before = [f.step_rows(i) for i in range(f.n_launches)]
    f.set_static_rows(96, 160)                              # accepted, and the plan stays un-windowed
    assert [f.step_rows(i) for i in range(f.n_launches)] == before and all(y0 == 0 for y0, _ in before)
    assert not any(" r[" in d for _, _, d in f._tunable)


# ---------------------------------------------------------------------------------------------------
# Detector
# ---------------------------------------------------------------------------------------------------
def detector_heads(out_path=None):
    """Two NV12 1080p surfaces for four ticks with changing content, then two 1440 x 1080 surfaces (content rows [80, 560)) for three:
    the head tensor of every tick.  Every convolution step runs variant 0 (the tuner is given nothing to time), so that two
    processes run the same kernels."""
    from realtime_video_analytics_32streams_amd.config import DetectorConfig
    from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
    os.environ["RVA_SKIP_VARIANTS"] = " ".join(str(v) for v in range(1, N.lib().rva_conv_num_variants() + 1))
    os.environ["RVA_TUNE_CACHE"] = "0"
    det = HipYoloDetector(DetectorConfig(model_path="yolov8s.pt", backend="hip", half=True, confidence_threshold=0.25, warmup=False))
    rng = np.random.default_rng(4)
    heads, rows = [], []
    for (w, h), ticks in (((1920, 1080), 4), ((1440, 1080), 3)):
        for _ in range(ticks):
            frames = [ops.Nv12Surface.from_numpy(rng.integers(16, 236, (h, w), dtype=np.uint8), rng.integers(16, 241, (h // 2, w), dtype=np.uint8), w, h)
                      for _ in range(2)]
            det.predict_batch_device([SimpleNamespace(frame=f) for f in frames])
            plan = det._plans[(2, 640, 640)]
            heads.append(plan.out.clone().cpu())
            rows.append((plan.static_rows, plan.step_rows(0)))
    torch.cuda.synchronize()
    if out_path:
        torch.save({"heads": heads, "rows": rows}, out_path)
    return heads, rows


def test_detector_heads_equal_the_unwindowed_process(tmp_path, monkeypatch):
    monkeypatch.delenv("RVA_PLAN_NO_STATIC_ROWS", raising=False)
    ref_file = tmp_path / "ref.pt"
    env = dict(os.environ, RVA_PLAN_NO_STATIC_ROWS="1", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    # a fresh child process: the switch is read by the library, and the reference must not share this process's plans
    child = subprocess.run([sys.executable, "-c", "import sys; from tests.test_gpu_static_rows import detector_heads; detector_heads(sys.argv[1])",
                            str(ref_file)], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stderr[-2000:]
    ref = torch.load(ref_file)
    with monkeypatch.context() as mp:
        mp.setenv("RVA_SKIP_VARIANTS", "")                   # detector_heads sets both: restored on the way out
        mp.setenv("RVA_TUNE_CACHE", "0")
        heads, rows = detector_heads()
    assert all(r == ((0, 640), (0, 160)) for r in ref["rows"]), ref["rows"]          # the reference never windowed
    assert [r[0] for r in rows] == [(140, 500)] * 4 + [(80, 560)] * 3 and all(r[1] != (0, 160) for r in rows), rows
    assert len(heads) == len(ref["heads"]) == 7
    for t, (got, want) in enumerate(zip(heads, ref["heads"])):
        assert torch.equal(_bits(got), _bits(want)), ("tick", t)
