"""The two YOLOv5 kernels against float64 references computed from the same fp16-rounded inputs and weights, within the bounds
derived in tests/yolov5_refs.py (never fitted to the kernels): ``rva_stem6_conv_f16`` (6x6 s2 p2 stem on K1's planar tensor) and
``rva_conv1x1_head5_f16`` (a level's 1x1 convolution fused with the anchor decode).  Every comparison prints max observed / bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from tests import yolov5_refs as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ------------------------------------------------------------------------------------------------------------------ stem
@functools.lru_cache(maxsize=None)
def _stem_inputs(hw, cout):
    rng = np.random.default_rng([3, hw[0], hw[1], cout])
    x = rng.uniform(0, 1, (3, 3, *hw)).astype(np.float16)              # what K1 writes: [0, 1]
    x[:, :, :3] = rng.uniform(0.5, 1, (3, 3, 3, hw[1]))                 # borders that matter
    w = rng.normal(0, 0.12, (cout, 3, 6, 6)).astype(np.float16)
    b = rng.normal(0, 0.3, cout).astype(np.float32)
    ref, mag = R.stem6_f64(x, w, b)
    return x, w, b, ref, R.stem6_bound(ref, mag)


def _pack_stem(w, b):
    cout = w.shape[0]
    wp = np.zeros((64, 128), dtype=np.float16)
    wp[:cout, :108] = w.reshape(cout, 108)
    return torch.from_numpy(wp).cuda(), torch.from_numpy(b).cuda()


def _run_stem(x, wd, bd, cout, rows=None, out=None):
    B, _, H, W = x.shape
    ldo, off = cout + 24, 8
    if out is None:
        out = torch.full((B, H // 2, W // 2, ldo), SENTINEL, dtype=torch.float16, device="cuda")
    ctx = ops.context()
    view = out[..., off:]
    if rows is None:
        rc = N.lib().rva_stem6_conv_f16(ctx.handle, _p(x), _p(wd), _p(bd), C.c_void_p(view.data_ptr()), ldo, B, H, W, cout, _stream())
    else:
        rc = N.lib().rva_stem6_conv_f16_rows(ctx.handle, _p(x), _p(wd), _p(bd), C.c_void_p(view.data_ptr()), ldo, B, H, W, cout, rows[0], rows[1], _stream())
    ctx.check(rc, "rva_stem6_conv_f16")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cout", [16, 32, 48, 64])
@pytest.mark.parametrize("hw", [(32, 32), (64, 96), (96, 40)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_stem6_against_float64(hw, cout):
    x, w, b, ref, tol = _stem_inputs(hw, cout)
    wd, bd = _pack_stem(w, b)
    bad = []
    outs = {}
    for B in (3, 1):
        xd = torch.from_numpy(x[:B]).cuda().contiguous()
        out = _run_stem(xd, wd, bd, cout)
        outs[B] = out
        got = out[..., 8:8 + cout].float().cpu().numpy()
        R.check("stem6", f"B {B} {hw[0]}x{hw[1]} Cout {cout}", got, ref[:B], tol[:B], bad)
        assert bool((out[..., :8] == SENTINEL).all()) and bool((out[..., 8 + cout:] == SENTINEL).all()), "wrote outside its channel slice"
    assert torch.equal(_bits(outs[1]), _bits(outs[3][:1])), "image 0 alone differs from image 0 of three"
    assert not bad, bad


def test_stem6_rows_are_the_bits_of_the_whole_launch():
    hw, cout = (96, 40), 32
    x, w, b, _, _ = _stem_inputs(hw, cout)
    wd, bd = _pack_stem(w, b)
    xd = torch.from_numpy(x[:2]).cuda().contiguous()
    whole = _run_stem(xd, wd, bd, cout)
    for y0, y1 in [(0, 48), (5, 6), (7, 30), (40, 48)]:
        part = _run_stem(xd, wd, bd, cout, rows=(y0, y1))
        assert torch.equal(_bits(part[:, y0:y1]), _bits(whole[:, y0:y1])), (y0, y1)
        assert bool((part[:, :y0] == SENTINEL).all()) and bool((part[:, y1:] == SENTINEL).all()), (y0, y1)
    ctx = ops.context()
    lib = N.lib()
    out = torch.empty((2, 48, 20, 32), dtype=torch.float16, device="cuda")
    for args in [(32, 2, 96, 40, 32, 10, 10), (32, 2, 96, 40, 32, 0, 49), (32, 2, 96, 44, 32, 0, -1), (32, 2, 96, 40, 72, 0, -1), (24, 2, 96, 40, 32, 0, -1)]:
        ldo, B, H, W, co, y0, y1 = args
        assert lib.rva_stem6_conv_f16_rows(ctx.handle, _p(xd), _p(wd), _p(bd), _p(out), ldo, B, H, W, co, y0, y1, _stream()) == N.RVA_ERR_ARG, args


# ------------------------------------------------------------------------------------------------------------------ head
def _head_inputs(family, B, h, w, cin, nc):
    """fp16 input [B,h,w,cin], fp16 weights [3*(5+nc), cin], fp32 bias.  ``wide``: logits spread over about +-20 (saturated
    sigmoids on both sides).  ``designed``: one-hot pixels select a weight column, so every logit is a designed value exactly:
    the grid -20 (1/16) 20, -0.0, ties between neighbouring entries, +-17, +-30.  The bounds are relative (2^-22 |ref| for
    ``boxes32``), so the logits stay where every fp32 intermediate is a normal number: below about -43 the square (2 y)^2
    underflows in fp32 and the side tensor holds 0 where float64 holds 1e-38 a -- true of any fp32 output, and not modelled."""
    rng = np.random.default_rng([9, ("wide", "designed").index(family), h, w, cin, nc])
    co = 3 * (5 + nc)
    if family == "wide":
        x = rng.normal(0, 1, (B, h, w, cin)).astype(np.float16)
        wt = (rng.normal(0, 1, (co, cin)) * (9.0 / np.sqrt(cin))).astype(np.float16)
        b = rng.normal(0, 2.0, co).astype(np.float32)
    else:
        x = np.zeros((B, h, w, cin), dtype=np.float16)
        pick = rng.integers(0, cin, (B, h, w))
        np.put_along_axis(x, pick[..., None], np.float16(1.0), axis=3)
        grid = np.concatenate([np.arange(-20, 20.0001, 1 / 16), [-0.0, 17.0, -17.0, 30.0, -30.0]])
        wt = rng.choice(grid, (co, cin))
        for r in range(1, co, 2):                                          # ties with the entry before
            m = rng.random(cin) < 0.3
            wt[r, m] = wt[r - 1, m]
        wt = wt.astype(np.float16)
        b = np.zeros(co, dtype=np.float32)
    return x, wt, b


def _run_head(x, wt, b, nc, anchors_lv, stride, A, a0, boxes, variant=0):
    B, h, w, cin = x.shape
    co = 3 * (5 + nc)
    cop = (co + 7) // 8 * 8
    cpad = int(N.lib().rva_conv_cout_pad(cop))
    wp = np.zeros((cpad, cin), dtype=np.float16)
    wp[:co] = wt
    bp = np.zeros(cpad, dtype=np.float32)
    bp[:co] = b
    xd, wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(wp).cuda(), torch.from_numpy(bp).cuda()
    ad = torch.tensor(np.asarray(anchors_lv, dtype=np.float32).reshape(6), device="cuda")
    out = torch.full((B, 5 + nc, A), SENTINEL, dtype=torch.float16, device="cuda")
    b32 = torch.full((B, 4, A), SENTINEL, dtype=torch.float32, device="cuda") if boxes else None
    ctx = ops.context()
    rc = N.lib().rva_conv1x1_head5_f16(ctx.handle, _p(xd), cin, _p(wd), _p(bd), B, h, w, cin, nc, _p(ad), _p(out),
                                       _p(b32) if boxes else None, A, a0, C.c_float(stride), variant, _stream())
    ctx.check(rc, "rva_conv1x1_head5_f16")
    torch.cuda.synchronize()
    return out, b32


@pytest.mark.parametrize("family", ["wide", "designed"])
@pytest.mark.parametrize("nc", [1, 3, 80])
@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("hw", [(2, 3), (5, 7), (20, 20)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_head5_against_float64(hw, cin, nc, family):
    B, (h, w) = 2, hw
    lv = (hw[0] + cin + nc) % 3
    anchors_lv, stride = R.DEFAULT_ANCHORS[lv], R.STRIDES[lv]
    x, wt, b = _head_inputs(family, B, h, w, cin, nc)
    z, mag = R.logits_f64(x, wt, b)
    if family == "wide":
        assert z.min() < -15 and z.max() > 15
    tol16, tol32, ref = R.head5_bound(z, mag, cin, anchors_lv, stride, nc)
    n, a0 = 3 * h * w, 21
    A = n + 37
    out, b32 = _run_head(x, wt, b, nc, anchors_lv, stride, A, a0, True)
    bad = []
    what = f"{family} {h}x{w} Cin {cin} nc {nc}"
    got = out[:, :, a0:a0 + n].float().cpu().numpy()
    R.check("head5 xy", what, got[:, :2], ref[:, :2], tol16[:, :2], bad)
    R.check("head5 wh", what, got[:, 2:4], ref[:, 2:4], tol16[:, 2:4], bad)
    R.check("head5 scores", what, got[:, 4:], ref[:, 4:], tol16[:, 4:], bad)
    g32 = b32[:, :, a0:a0 + n].cpu().numpy()
    R.check("head5 boxes32 xy", what, g32[:, :2], ref[:, :2], tol32[:, :2], bad)
    R.check("head5 boxes32 wh", what, g32[:, 2:], ref[:, 2:4], tol32[:, 2:], bad)
    assert torch.equal(_bits(b32[:, :, a0:a0 + n].half()), _bits(out[:, :4, a0:a0 + n])), "(half)boxes32 != rows 0-3"
    for t in (out, b32):
        assert bool((t[:, :, :a0] == SENTINEL).all()) and bool((t[:, :, a0 + n:] == SENTINEL).all()), "wrote outside the level's anchors"
    # without the side tensor: the same head; one image alone: the bits of the same image inside two
    plain, _ = _run_head(x, wt, b, nc, anchors_lv, stride, A, a0, False)
    assert torch.equal(_bits(plain), _bits(out))
    one, _ = _run_head(x[1:], wt, b, nc, anchors_lv, stride, A, a0, False)
    assert torch.equal(_bits(one[0]), _bits(out[1])), "B = 1 differs from the same image inside B = 2"
    assert not bad, bad


def test_head5_gather_variants_and_refusals():
    """Every tile of the gather-64 family computes each logit in fp32 from the same 64-channel K-steps in the same order."""
    B, h, w, cin, nc = 2, 20, 20, 128, 80
    anchors_lv, stride = R.DEFAULT_ANCHORS[0], 8.0
    x, wt, b = _head_inputs("wide", B, h, w, cin, nc)
    n = 3 * h * w
    base, _ = _run_head(x, wt, b, nc, anchors_lv, stride, n, 0, False)
    for v in range(33, 40):
        got, _ = _run_head(x, wt, b, nc, anchors_lv, stride, n, 0, False, variant=v)
        assert torch.equal(_bits(got), _bits(base)), v
    ctx, lib = ops.context(), N.lib()
    t = torch.zeros(64 * 1024, dtype=torch.float16, device="cuda")
    f = torch.zeros(64, dtype=torch.float32, device="cuda")
    for cin_, nc_, A_, a0_, var in [(96, 3, 100, 0, 0), (64, 0, 100, 0, 0), (64, 1025, 100000, 0, 0), (64, 3, 17, 0, 0), (64, 3, 100, 90, 0), (64, 3, 100, 0, 5)]:
        rc = lib.rva_conv1x1_head5_f16(ctx.handle, _p(t), cin_, _p(t), _p(f), 1, 2, 3, cin_, nc_, _p(f), _p(t), None, A_, a0_, C.c_float(8.0), var, _stream())
        assert rc == N.RVA_ERR_ARG, (cin_, nc_, A_, a0_, var)
    torch.cuda.synchronize()
