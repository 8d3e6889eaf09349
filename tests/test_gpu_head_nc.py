"""The detect head for any class count: ``rva_yolo_head_nc_f16``, ``rva_yolo_head3_nc_f16`` and ``rva_conv1x1_head_nc_f16`` against
float64, through the C ABI.

Reference, logit sets and per-element bounds are those of tests/head_refs.py, unchanged; the device helpers are those of
tests/test_gpu_head_f64.py.  What is new here is the ragged class count: nc = 1 (the 5-row head the post-process reads as plain
scores), 3, 12 (one full group of eight and a ragged one) and 91 (the interior width follows the class count), class rows of
ldc = roundup(nc, 8) or more halves whose pad columns hold NaN, and an output of exactly 4 + nc rows per image -- with an odd 4 + nc
the first row of the next image sits right behind the last class row, so a class row stored past nc lands in it.  Every output is
allocated one image larger than the batch and pre-filled with a sentinel: nothing but the level's anchors of rows 0 .. 4+nc-1 of
the batch's images may change."""
import ctypes as C

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from tests import head_refs as R
from tests.test_gpu_head_f64 import SENTINEL, _accepted, _boxes32, _case, _fill, _identity_conv, _level, _ptr, _stream

pytestmark = pytest.mark.gpu

NCS = [1, 3, 12, 91]
LAYOUTS = ["packed", "wide"]


def _up8(n):
    return (n + 7) // 8 * 8


def _place_nc(box, cls, layout):
    """The logits on the device with NaN in every column that is not a logit -> (keep alive, box pointer, ldb, class pointer, ldc).
    packed: box rows of 64, class rows of roundup(nc, 8); wide: both are slices of one row of 64 + roundup(nc, 8) + 8 halves."""
    box, cls = torch.from_numpy(box), torch.from_numpy(cls)
    nc = cls.shape[3]
    if layout == "packed":
        c = torch.full((*cls.shape[:3], _up8(nc)), float("nan"), dtype=torch.float16)
        c[..., :nc] = cls
        b, c = box.cuda(), c.cuda()
        return (b, c), _ptr(b), 64, _ptr(c), _up8(nc)
    ld = 64 + _up8(nc) + 8
    row = torch.full((*box.shape[:3], ld), float("nan"), dtype=torch.float16)
    row[..., :64], row[..., 64:64 + nc] = box, cls
    row = row.cuda()
    return (row,), _ptr(row), ld, _ptr(row, 64), ld


def _batch_only(out, B, what):
    """The batch's images of an output allocated one image larger, after asserting that the extra image still holds its fill."""
    extra = out[B]
    untouched = torch.isnan(extra).all() if extra.dtype == torch.float32 else (extra == SENTINEL).all()
    assert bool(untouched), (what, "written behind the last image")
    return out[:B]


# ------------------------------------------------------------------------------------------------ head_anchor, one level
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=R.geometry_id)
def test_head_nc_against_float64(geometry, nc, layout):
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w = geometry
    hw, stride = h * w, R.GEOMETRY_STRIDE[geometry]
    A = hw + R.PAD_ANCHORS
    bad = []
    for name in R.BOX_SETS:
        box, cls, ref, tol = _case(name, geometry, nc, "f16", stride)
        keep, bp, ldb, cp, ldc = _place_nc(box, cls, layout)
        what = f"{R.geometry_id(geometry)} nc {nc} {layout} {name}"
        out = _fill((B + 1, 4 + nc, A), torch.float16)
        ctx.check(L.rva_yolo_head_nc_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(out), None, B, h, w, nc, A, R.A0, C.c_float(stride), s),
                  "rva_yolo_head_nc_f16")
        out2, b32 = _fill((B + 1, 4 + nc, A), torch.float16), _fill((B + 1, 4, A), torch.float32, float("nan"))
        ctx.check(L.rva_yolo_head_nc_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(out2), _ptr(b32), B, h, w, nc, A, R.A0, C.c_float(stride), s),
                  "rva_yolo_head_nc_f16")
        torch.cuda.synchronize()
        assert torch.equal(out, out2), what
        got = _level(_batch_only(out, B, what), R.A0, hw, what)
        assert np.isfinite(got).all(), (what, "a pad column of the class logits reached the output")
        tol16 = R.fp16_store_tol(ref, tol)
        R.check_rows("rva_yolo_head_nc_f16", what, got, ref, tol16, bad)
        R.check("rva_yolo_head_nc_f16 boxes32", what, _boxes32(_batch_only(b32, B, what), out2[:B], R.A0, hw, what), ref[:, :4], tol[:, :4], bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ head_anchor, three levels in one launch
def _head3_args(placed, levels):
    bp, k1 = N.ptr_array([p[1].value for p in placed])
    cp, k2 = N.ptr_array([p[3].value for p in placed])
    ldb, k3 = N.i32_array([p[2] for p in placed])
    ldc, k4 = N.i32_array([p[4] for p in placed])
    hp, k5 = N.i32_array([h for h, _ in levels])
    wp, k6 = N.i32_array([w for _, w in levels])
    return (bp, ldb, cp, ldc, hp, wp), (k1, k2, k3, k4, k5, k6)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("levels", R.HEAD3_CASES, ids=["tails", "exact-blocks"])
def test_head3_nc_against_float64(levels, nc, layout):
    L, ctx, s = N.lib(), ops.context(), _stream()
    B = 2
    A3 = sum(h * w for h, w in levels)
    sp = (C.c_float * 3)(*R.STRIDES)
    bad = []
    for name in ("mixed", "offset"):
        cases = [_case(name, (B, h, w), nc, "f16", st) for (h, w), st in zip(levels, R.STRIDES)]
        placed = [_place_nc(c[0], c[1], layout) for c in cases]
        ref, tol = np.concatenate([c[2] for c in cases], 2), np.concatenate([c[3] for c in cases], 2)
        (bp, ldb, cp, ldc, hp, wp), _keep = _head3_args(placed, levels)
        what = f"{'+'.join(R.geometry_id(l) for l in levels)} x{B} nc {nc} {layout} {name}"
        out = _fill((B + 1, 4 + nc, A3), torch.float16)
        ctx.check(L.rva_yolo_head3_nc_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(out), None, B, hp, wp, nc, A3, sp, s), "rva_yolo_head3_nc_f16")
        out2, b32 = _fill((B + 1, 4 + nc, A3), torch.float16), _fill((B + 1, 4, A3), torch.float32, float("nan"))
        ctx.check(L.rva_yolo_head3_nc_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(out2), _ptr(b32), B, hp, wp, nc, A3, sp, s), "rva_yolo_head3_nc_f16")
        torch.cuda.synchronize()
        assert torch.equal(out, out2), what
        got = _batch_only(out, B, what).double().cpu().numpy()
        assert np.isfinite(got).all(), (what, "a pad column of the class logits reached the output")
        R.check_rows("rva_yolo_head3_nc_f16", what, got, ref, R.fp16_store_tol(ref, tol), bad)
        R.check("rva_yolo_head3_nc_f16 boxes32", what, _boxes32(_batch_only(b32, B, what), out2[:B], 0, A3, what), ref[:, :4], tol[:, :4], bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the fused epilogue
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=R.geometry_id)
def test_fused_box_epilogue_nc_against_float64(geometry, nc):
    """Mode 1 (Cin = Cout = 64) of rva_conv1x1_head_nc_f16, every variant it accepts, with and without the side tensor: the image
    stride of the output is (4 + nc) * A for any nc."""
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w = geometry
    hw, stride = h * w, R.GEOMETRY_STRIDE[geometry]
    A = hw + R.PAD_ANCHORS
    box, cls, ref, tol = _case("mixed", geometry, nc, "f16", stride)
    x, wt, bias = _identity_conv(box, 64)
    ref, tol = ref[:, :4], tol[:, :4]
    tol16 = R.fp16_store_tol(ref, tol)

    def run(v, out, b32=None):
        return L.rva_conv1x1_head_nc_f16(ctx.handle, _ptr(x), 64, _ptr(wt), _ptr(bias), B, h, w, 64, 64, 1, _ptr(out),
                                         _ptr(b32) if b32 is not None else None, nc, A, R.A0, C.c_float(stride), v, s)
    probe = _fill((B + 1, 4 + nc, A), torch.float16)
    bad = []
    for v in _accepted(lambda v: run(v, probe)):
        what = f"{R.geometry_id(geometry)} nc {nc} variant {v}"
        out = _fill((B + 1, 4 + nc, A), torch.float16)
        ctx.check(run(v, out), "rva_conv1x1_head_nc_f16")
        out2, b32 = _fill((B + 1, 4 + nc, A), torch.float16), _fill((B + 1, 4, A), torch.float32, float("nan"))
        ctx.check(run(v, out2, b32), "rva_conv1x1_head_nc_f16")
        torch.cuda.synchronize()
        assert torch.equal(out, out2), what
        R.check("rva_conv1x1_head_nc_f16 mode 1 box", what, _level(_batch_only(out, B, what), R.A0, hw, what, slice(0, 4)), ref, tol16, bad)
        R.check("rva_conv1x1_head_nc_f16 boxes32", what, _boxes32(_batch_only(b32, B, what), out2[:B], R.A0, hw, what), ref, tol, bad)
    assert not bad, bad


def _padded_cls(cls, fill=7.0):
    """[B, h, w, nc] -> [B, h, w, roundup(nc, 8)]: what the convolution's pad output channels deliver is a finite value the decode
    must drop (a NaN cannot be fed through a convolution without reaching every channel)."""
    nc = cls.shape[3]
    out = np.full((*cls.shape[:3], _up8(nc)), fill, dtype=np.float16)
    out[..., :nc] = cls
    return out


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=R.geometry_id)
def test_fused_class_epilogue_nc_against_float64(geometry, nc):
    """Mode 2 (Cin = 128, Cout = roundup(nc, 8); 91 -> 96: two column tiles, the second one ragged) of rva_conv1x1_head_nc_f16, every
    variant: class rows < nc against float64, nothing else written."""
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w = geometry
    hw, stride = h * w, R.GEOMETRY_STRIDE[geometry]
    A = hw + R.PAD_ANCHORS
    box, cls, ref, tol = _case("mixed", geometry, nc, "f16", stride)
    x, wt, bias = _identity_conv(_padded_cls(cls), 128)
    ref, tol = ref[:, 4:], tol[:, 4:]
    tol16 = R.fp16_store_tol(ref, tol)

    def run(v, out):
        return L.rva_conv1x1_head_nc_f16(ctx.handle, _ptr(x), 128, _ptr(wt), _ptr(bias), B, h, w, 128, _up8(nc), 2, _ptr(out), None, nc, A, R.A0,
                                         C.c_float(stride), v, s)
    probe = _fill((B + 1, 4 + nc, A), torch.float16)
    bad = []
    for v in _accepted(lambda v: run(v, probe)):
        what = f"{R.geometry_id(geometry)} nc {nc} variant {v}"
        out = _fill((B + 1, 4 + nc, A), torch.float16)
        ctx.check(run(v, out), "rva_conv1x1_head_nc_f16")
        torch.cuda.synchronize()
        R.check("rva_conv1x1_head_nc_f16 mode 2 scores", what, _level(_batch_only(out, B, what), R.A0, hw, what, slice(4, 4 + nc)), ref, tol16, bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ nc % 8 == 0: the existing entries' bits
@pytest.mark.parametrize("nc", [8, 80])
def test_nc_entries_are_bit_identical_to_the_existing_ones(nc):
    L, ctx, s = N.lib(), ops.context(), _stream()
    geometry = R.GEOMETRIES[0]
    B, h, w = geometry
    hw, stride = h * w, R.GEOMETRY_STRIDE[geometry]
    A = hw + R.PAD_ANCHORS
    box, cls, _, _ = _case("mixed", geometry, nc, "f16", stride)
    keep, bp, ldb, cp, ldc = _place_nc(box, cls, "wide")
    shape = (B, 4 + nc, A)
    # one level
    old, new = _fill(shape, torch.float16), _fill(shape, torch.float16)
    old32, new32 = _fill((B, 4, A), torch.float32), _fill((B, 4, A), torch.float32)
    ctx.check(L.rva_yolo_head_box32_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(old), _ptr(old32), B, h, w, nc, A, R.A0, C.c_float(stride), s), "old")
    ctx.check(L.rva_yolo_head_nc_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(new), _ptr(new32), B, h, w, nc, A, R.A0, C.c_float(stride), s), "new")
    torch.cuda.synchronize()
    assert torch.equal(old, new) and torch.equal(old32, new32) and not bool((new[:, :, R.A0:R.A0 + hw] == SENTINEL).any())
    # three levels
    levels = R.HEAD3_CASES[0]
    A3 = sum(a * b for a, b in levels)
    cases = [_case("mixed", (2, a, b), nc, "f16", st) for (a, b), st in zip(levels, R.STRIDES)]
    placed = [_place_nc(c[0], c[1], "packed") for c in cases]
    (bp3, ldb3, cp3, ldc3, hp, wp), _keep = _head3_args(placed, levels)
    sp = (C.c_float * 3)(*R.STRIDES)
    old, new = _fill((2, 4 + nc, A3), torch.float16), _fill((2, 4 + nc, A3), torch.float16)
    ctx.check(L.rva_yolo_head3_f16(ctx.handle, bp3, ldb3, cp3, ldc3, _ptr(old), 2, hp, wp, nc, A3, sp, s), "old")
    ctx.check(L.rva_yolo_head3_nc_f16(ctx.handle, bp3, ldb3, cp3, ldc3, _ptr(new), None, 2, hp, wp, nc, A3, sp, s), "new")
    torch.cuda.synchronize()
    assert torch.equal(old, new) and not bool((new == SENTINEL).any())
    # the fused epilogue, both modes, the heuristic and one explicit variant
    xb, wb, bb = _identity_conv(box, 64)
    xc, wc, bc = _identity_conv(cls, 128)
    for v in (0, 33):
        old, new = _fill(shape, torch.float16), _fill(shape, torch.float16)
        old32, new32 = _fill((B, 4, A), torch.float32), _fill((B, 4, A), torch.float32)
        ctx.check(L.rva_conv1x1_head_box32_f16(ctx.handle, _ptr(xb), 64, _ptr(wb), _ptr(bb), B, h, w, 64, _ptr(old), _ptr(old32), nc, A, R.A0,
                                               C.c_float(stride), v, s), "old")
        ctx.check(L.rva_conv1x1_head_f16(ctx.handle, _ptr(xc), 128, _ptr(wc), _ptr(bc), B, h, w, 128, nc, 2, _ptr(old), nc, A, R.A0,
                                         C.c_float(stride), v, s), "old")
        ctx.check(L.rva_conv1x1_head_nc_f16(ctx.handle, _ptr(xb), 64, _ptr(wb), _ptr(bb), B, h, w, 64, 64, 1, _ptr(new), _ptr(new32), nc, A, R.A0,
                                            C.c_float(stride), v, s), "new")
        ctx.check(L.rva_conv1x1_head_nc_f16(ctx.handle, _ptr(xc), 128, _ptr(wc), _ptr(bc), B, h, w, 128, nc, 2, _ptr(new), None, nc, A, R.A0,
                                            C.c_float(stride), v, s), "new")
        torch.cuda.synchronize()
        assert torch.equal(old, new) and torch.equal(old32, new32), v
        assert not bool((new[:, :, R.A0:R.A0 + hw] == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ refused calls
def test_bad_nc_arguments_are_refused_before_any_launch():
    """Each bad call returns RVA_ERR_ARG and leaves the sentinel in place.  As in tests/test_gpu_head_f64.py the buffers are larger
    than anything a call declares, so a library without a check would still write inside them: the test fails by the return code
    and the sentinel, never by a fault."""
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w, nc = 2, 20, 13, 3
    hw = h * w
    A = hw + R.PAD_ANCHORS
    box = torch.zeros((B, h, w, 144), dtype=torch.float16, device="cuda")
    cls = torch.zeros((B, h, w, 144), dtype=torch.float16, device="cuda")
    out = _fill((B, 4 + 1040, 2 * A), torch.float16)
    b32 = _fill((B, 4, 2 * A), torch.float32)
    good = dict(ldb=64, ldc=8, batch=B, h=h, w=w, nc=nc, A=A, a0=R.A0)

    def head(**kw):
        a = {**good, **kw}
        return L.rva_yolo_head_nc_f16(ctx.handle, _ptr(box), a["ldb"], _ptr(cls), a["ldc"], _ptr(out), _ptr(b32), a["batch"], a["h"], a["w"],
                                      a["nc"], a["A"], a["a0"], C.c_float(8.0), s)
    bad_calls = [dict(nc=0), dict(nc=-8), dict(nc=1025), dict(nc=9), dict(nc=12, ldc=8), dict(ldc=12), dict(ldc=0), dict(ldb=68),
                 dict(batch=0), dict(h=0), dict(w=-1), dict(a0=-1), dict(a0=A - hw + 1), dict(A=hw - 1, a0=0)]
    for kw in bad_calls:
        assert head(**kw) == N.RVA_ERR_ARG, kw
    levels = R.HEAD3_CASES[0]
    A3 = sum(a * b for a, b in levels)
    ptrs, _k1 = N.ptr_array([box.data_ptr()] * 3)
    cptrs, _k2 = N.ptr_array([cls.data_ptr()] * 3)
    ld, _k3 = N.i32_array([64] * 3)
    ldc, _k4 = N.i32_array([8] * 3)
    ldc_bad, _k5 = N.i32_array([8, 12, 8])
    hp, _k6 = N.i32_array([a for a, _ in levels])
    wp, _k7 = N.i32_array([b for _, b in levels])
    sp = (C.c_float * 3)(*R.STRIDES)
    for total, ldcs, ncs, bt in ((A3 - 1, ldc, nc, 1), (A3 + 1, ldc, nc, 1), (A3, ldc_bad, nc, 1), (A3, ldc, 0, 1), (A3, ldc, 9, 1),
                                 (A3, ldc, 1025, 1), (A3, ldc, nc, 0)):
        assert L.rva_yolo_head3_nc_f16(ctx.handle, ptrs, ld, cptrs, ldcs, _ptr(out), _ptr(b32), bt, hp, wp, ncs, total, sp, s) == N.RVA_ERR_ARG
    x = torch.zeros((B, h, w, 128), dtype=torch.float16, device="cuda")
    wt = torch.zeros((128, 1, 128), dtype=torch.float16, device="cuda")
    bias = torch.zeros(128, dtype=torch.float32, device="cuda")
    fgood = dict(Cin=128, Cout=8, mode=2, b32=None, nc=nc, A=A, a0=R.A0, ldi=128)

    def fused(**kw):
        a = {**fgood, **kw}
        return L.rva_conv1x1_head_nc_f16(ctx.handle, _ptr(x), a["ldi"], _ptr(wt), _ptr(bias), B, h, w, a["Cin"], a["Cout"], a["mode"], _ptr(out),
                                         a["b32"], a["nc"], a["A"], a["a0"], C.c_float(8.0), 0, s)
    for kw in [dict(nc=0), dict(nc=1025), dict(Cout=16), dict(Cout=3), dict(nc=9), dict(nc=12), dict(mode=0), dict(mode=3),
               dict(mode=1, Cout=8), dict(b32=_ptr(b32)), dict(Cin=96), dict(ldi=100), dict(a0=-1), dict(a0=A - hw + 1), dict(A=hw - 1, a0=0)]:
        assert fused(**kw) == N.RVA_ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((b32 == SENTINEL).all())
    # the good calls are accepted and write the level's 4 + nc rows alone
    ctx.check(head(), "rva_yolo_head_nc_f16")
    torch.cuda.synchronize()
    flat = out.flatten().cpu()
    used = flat[:B * (4 + nc) * A].view(B, 4 + nc, A)
    assert bool((used[:, :, R.A0:R.A0 + hw] != SENTINEL).all()) and bool((flat[B * (4 + nc) * A:] == SENTINEL).all())
    assert bool((used[:, :, :R.A0] == SENTINEL).all()) and bool((used[:, :, R.A0 + hw:] == SENTINEL).all())
    out.fill_(SENTINEL)
    ctx.check(fused(), "rva_conv1x1_head_nc_f16")
    torch.cuda.synchronize()
    flat = out.flatten().cpu()
    used = flat[:B * (4 + nc) * A].view(B, 4 + nc, A)
    assert bool((used[:, 4:, R.A0:R.A0 + hw] == 0.5).all()) and bool((used[:, :4] == SENTINEL).all())
    assert bool((flat[B * (4 + nc) * A:] == SENTINEL).all())
