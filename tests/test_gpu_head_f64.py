"""The detect head's three copies against float64 on peaked, tied, offset and saturated logits, through the C ABI:
``head_anchor`` (rva_yolo_head_f16, rva_yolo_head3_f16 and their _box32 forms), the ``HEAD`` epilogue of the 1x1 convolution
(rva_conv1x1_head_f16, rva_conv1x1_head_box32_f16) and ``k_head_f32`` (rva_yolo_head_f32).

Reference, logit sets and per-element bounds: tests/head_refs.py (derived from the number formats, never from a kernel's output);
tests/test_head_refs_host.py proves on the CPU that those bounds see the head's bug classes.  Every written element is compared, and
everything outside the level's anchor range must still hold the sentinel the output was filled with.

Geometries (thread per anchor, 256 per block, grid.y = batch): 3x20x13 (a full block and a tail of 4, h != w), 1x1x1, 2x16x16
(exactly one block), 2x5x77; A = h*w + 37 anchors with the level at offset 21; row strides 64 / nc (packed) and 144 / 144 (box and class
slices of one [.., 64 + 80] row, as the plan lays its detect buffers out).

Observed / bound: every test prints it per comparison (``pytest -s``); the largest per entry point is in profiles/head_f64.json and
DESIGN.md section 2.  A ratio above 1 is a finding about the kernel, not about the bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from tests import head_refs as R

pytestmark = pytest.mark.gpu

SENTINEL = -3.0
LAYOUTS = ["packed", "wide"]
FUSED_VARIANTS = [0] + list(range(33, 40))        # what test_head_fused_conv_is_bit_identical_to_conv_then_head lists


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


@functools.lru_cache(maxsize=None)
def _case(name, geometry, nc, kind, stride):
    return R.case(name, geometry, nc, kind, stride)


def _place(box, cls, layout):
    """The logits on the device -> (tensors to keep alive, box pointer, ldb, class pointer, ldc)."""
    box, cls = torch.from_numpy(box), torch.from_numpy(cls)
    nc = cls.shape[3]
    if layout == "packed":
        b, c = box.cuda(), cls.cuda()
        return (b, c), _ptr(b), 64, _ptr(c), nc
    row = torch.full((*box.shape[:3], 144), 5.0, dtype=box.dtype)
    row[..., :64], row[..., 64:64 + nc] = box, cls
    row = row.cuda()
    return (row,), _ptr(row), 144, _ptr(row, 64), 144


def _level(out, a0, hw, what, rows=slice(None)):
    """The level's slice of a sentinel-filled output, after asserting that nothing else was written."""
    out = out.cpu()
    written = torch.zeros_like(out, dtype=torch.bool)
    written[:, rows, a0:a0 + hw] = True
    assert bool((out[~written] == SENTINEL).all()), (what, "written outside the level's rows / anchor range")
    return out[:, rows, a0:a0 + hw].double().numpy()


def _boxes32(b32, out16, a0, hw, what):
    """The side tensor's level after asserting NaN outside it and ``boxes32.half()`` == rows 0-3 of the fp16 tensor, bit for bit."""
    b32, out16 = b32.cpu(), out16.cpu()
    outside = torch.ones_like(b32, dtype=torch.bool)
    outside[:, :, a0:a0 + hw] = False
    assert bool(torch.isnan(b32[outside]).all()), (what, "boxes32 written outside the level's anchor range")
    lv = b32[:, :, a0:a0 + hw]
    assert torch.equal(lv.half().contiguous().view(torch.int16), out16[:, :4, a0:a0 + hw].contiguous().view(torch.int16)), \
        (what, "boxes32 rounded to fp16 != the fp16 box rows")
    return lv.double().numpy()


def _fill(shape, dtype, value=SENTINEL):
    return torch.full(shape, value, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ head_anchor, one level
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nc", [8, 80])
@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=R.geometry_id)
def test_head_f16_against_float64(geometry, nc, layout):
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w = geometry
    hw, stride = h * w, R.GEOMETRY_STRIDE[geometry]
    A = hw + R.PAD_ANCHORS
    bad = []
    for name in R.BOX_SETS:
        box, cls, ref, tol = _case(name, geometry, nc, "f16", stride)
        keep, bp, ldb, cp, ldc = _place(box, cls, layout)
        what = f"{R.geometry_id(geometry)} nc {nc} {layout} {name}"
        out = _fill((B, 4 + nc, A), torch.float16)
        ctx.check(L.rva_yolo_head_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(out), B, h, w, nc, A, R.A0, C.c_float(stride), s), "rva_yolo_head_f16")
        out2, b32 = _fill((B, 4 + nc, A), torch.float16), _fill((B, 4, A), torch.float32, float("nan"))
        ctx.check(L.rva_yolo_head_box32_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(out2), _ptr(b32), B, h, w, nc, A, R.A0, C.c_float(stride), s),
                  "rva_yolo_head_box32_f16")
        torch.cuda.synchronize()
        tol16 = R.fp16_store_tol(ref, tol)
        R.check_rows("rva_yolo_head_f16", what, _level(out, R.A0, hw, what), ref, tol16, bad)
        R.check_rows("rva_yolo_head_box32_f16", what, _level(out2, R.A0, hw, what), ref, tol16, bad)
        R.check("rva_yolo_head_box32_f16 boxes32", what, _boxes32(b32, out2, R.A0, hw, what), ref[:, :4], tol[:, :4], bad)
        assert torch.equal(out, out2), what
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ k_head_f32
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nc", [1, 3, 80])
@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=R.geometry_id)
def test_head_f32_against_float64(geometry, nc, layout):
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w = geometry
    hw, stride = h * w, R.GEOMETRY_STRIDE[geometry]
    A = hw + R.PAD_ANCHORS
    bad = []
    for name in R.BOX_SETS:
        box, cls, ref, tol = _case(name, geometry, nc, "f32", stride)
        keep, bp, ldb, cp, ldc = _place(box, cls, layout)
        what = f"{R.geometry_id(geometry)} nc {nc} {layout} {name}"
        out = _fill((B, 4 + nc, A), torch.float32)
        ctx.check(L.rva_yolo_head_f32(ctx.handle, bp, ldb, cp, ldc, _ptr(out), B, h, w, nc, A, R.A0, C.c_float(stride), s), "rva_yolo_head_f32")
        torch.cuda.synchronize()
        R.check_rows("rva_yolo_head_f32", what, _level(out, R.A0, hw, what), ref, tol, bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ head_anchor, three levels in one launch
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("levels", R.HEAD3_CASES, ids=["tails", "exact-blocks"])
def test_head3_f16_against_float64(levels, layout):
    """(20,13), (10,7), (5,4): 2 + 1 + 1 blocks, a tail on every level, so a block mapped to the wrong level or a level's tail run
    with another level's bound shows; (16,16), (8,8), (4,4): a level boundary on a block boundary."""
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, nc = 2, 80
    A3 = sum(h * w for h, w in levels)
    bad = []
    for name in R.BOX_SETS:
        cases = [_case(name, (B, h, w), nc, "f16", st) for (h, w), st in zip(levels, R.STRIDES)]
        placed = [_place(c[0], c[1], layout) for c in cases]
        ref, tol = np.concatenate([c[2] for c in cases], 2), np.concatenate([c[3] for c in cases], 2)
        bp, _k1 = N.ptr_array([p[1].value for p in placed])
        cp, _k2 = N.ptr_array([p[3].value for p in placed])
        ldb, _k3 = N.i32_array([p[2] for p in placed])
        ldc, _k4 = N.i32_array([p[4] for p in placed])
        hp, _k5 = N.i32_array([h for h, _ in levels])
        wp, _k6 = N.i32_array([w for _, w in levels])
        sp = (C.c_float * 3)(*R.STRIDES)
        what = f"{'+'.join(R.geometry_id(l) for l in levels)} x{B} nc {nc} {layout} {name}"
        # one image more than the batch: the launch must leave it alone
        out = _fill((B + 1, 4 + nc, A3), torch.float16)
        ctx.check(L.rva_yolo_head3_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(out), B, hp, wp, nc, A3, sp, s), "rva_yolo_head3_f16")
        out2, b32 = _fill((B + 1, 4 + nc, A3), torch.float16), _fill((B + 1, 4, A3), torch.float32, float("nan"))
        ctx.check(L.rva_yolo_head3_box32_f16(ctx.handle, bp, ldb, cp, ldc, _ptr(out2), _ptr(b32), B, hp, wp, nc, A3, sp, s),
                  "rva_yolo_head3_box32_f16")
        torch.cuda.synchronize()
        assert bool((out[B] == SENTINEL).all()) and bool((out2[B] == SENTINEL).all()) and bool(torch.isnan(b32[B]).all()), what
        tol16 = R.fp16_store_tol(ref, tol)
        R.check_rows("rva_yolo_head3_f16", what, out[:B].double().cpu().numpy(), ref, tol16, bad)
        R.check_rows("rva_yolo_head3_box32_f16", what, out2[:B].double().cpu().numpy(), ref, tol16, bad)
        R.check("rva_yolo_head3_box32_f16 boxes32", what, _boxes32(b32[:B], out2[:B], 0, A3, what), ref[:, :4], tol[:, :4], bad)
        assert torch.equal(out, out2), what
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the fused epilogue
def _identity_conv(logits, Cin):
    """Activations, weights and bias through which a 1x1 convolution reproduces ``logits [B, h, w, Cout]`` exactly: the logits are
    the first Cout of Cin input channels (the rest hold 3.0 and meet zero weights), the weights an identity of fp16 1.0, the bias 0."""
    B, h, w, Cout = logits.shape
    cpad = N.lib().rva_conv_cout_pad(Cout)
    x = torch.full((B, h, w, Cin), 3.0, dtype=torch.float16)
    x[..., :Cout] = torch.from_numpy(logits)
    wt = torch.zeros((cpad, 1, Cin), dtype=torch.float16)
    wt[torch.arange(Cout), 0, torch.arange(Cout)] = 1.0
    return x.cuda(), wt.cuda(), torch.zeros(cpad, dtype=torch.float32, device="cuda")


def _accepted(call):
    """The variants 0 .. rva_conv_num_variants() an entry runs; every other one is refused with RVA_ERR_ARG."""
    ok = []
    for v in range(N.lib().rva_conv_num_variants() + 1):
        rc = call(v)
        assert rc in (N.RVA_OK, N.RVA_ERR_ARG), (v, rc)
        if rc == N.RVA_OK:
            ok.append(v)
    torch.cuda.synchronize()
    assert set(FUSED_VARIANTS) <= set(ok), ok
    return ok


@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=R.geometry_id)
def test_fused_box_epilogue_against_float64(geometry):
    """Mode 1 (Cin = Cout = 64) of rva_conv1x1_head_f16 and rva_conv1x1_head_box32_f16, every variant they accept: the staged tile is
    the designed logits bit for bit, so what is compared is the epilogue's decode alone -- against float64, not against head_anchor."""
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w = geometry
    hw, stride, nc = h * w, R.GEOMETRY_STRIDE[geometry], 80
    A = hw + R.PAD_ANCHORS
    bad, variants = [], None
    for name in R.BOX_SETS:
        box, cls, ref, tol = _case(name, geometry, nc, "f16", stride)
        x, wt, bias = _identity_conv(box, 64)
        ref, tol = ref[:, :4], tol[:, :4]
        tol16 = R.fp16_store_tol(ref, tol)

        def plain(v, out):
            return L.rva_conv1x1_head_f16(ctx.handle, _ptr(x), 64, _ptr(wt), _ptr(bias), B, h, w, 64, 64, 1, _ptr(out), nc, A, R.A0,
                                          C.c_float(stride), v, s)

        def side(v, out, b32):
            return L.rva_conv1x1_head_box32_f16(ctx.handle, _ptr(x), 64, _ptr(wt), _ptr(bias), B, h, w, 64, _ptr(out), _ptr(b32), nc, A, R.A0,
                                                C.c_float(stride), v, s)
        if variants is None:
            probe, probe32 = _fill((B, 4 + nc, A), torch.float16), _fill((B, 4, A), torch.float32)
            variants = _accepted(lambda v: plain(v, probe))
            assert _accepted(lambda v: side(v, probe, probe32)) == variants
        for v in variants:
            what = f"{R.geometry_id(geometry)} variant {v} {name}"
            out = _fill((B, 4 + nc, A), torch.float16)
            ctx.check(plain(v, out), "rva_conv1x1_head_f16")
            out2, b32 = _fill((B, 4 + nc, A), torch.float16), _fill((B, 4, A), torch.float32, float("nan"))
            ctx.check(side(v, out2, b32), "rva_conv1x1_head_box32_f16")
            torch.cuda.synchronize()
            R.check("rva_conv1x1_head_f16 mode 1 box", what, _level(out, R.A0, hw, what, slice(0, 4)), ref, tol16, bad)
            R.check("rva_conv1x1_head_box32_f16 box", what, _level(out2, R.A0, hw, what, slice(0, 4)), ref, tol16, bad)
            R.check("rva_conv1x1_head_box32_f16 boxes32", what, _boxes32(b32, out2, R.A0, hw, what), ref, tol, bad)
            assert torch.equal(out, out2), what
    assert not bad, bad


@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=R.geometry_id)
def test_fused_class_epilogue_against_float64(geometry):
    """Mode 2 (Cin = 128, Cout = nc = 80: two column tiles of 64, the second one ragged) of rva_conv1x1_head_f16, every variant."""
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w = geometry
    hw, stride, nc = h * w, R.GEOMETRY_STRIDE[geometry], 80
    A = hw + R.PAD_ANCHORS
    box, cls, ref, tol = _case("mixed", geometry, nc, "f16", stride)
    x, wt, bias = _identity_conv(cls, 128)
    ref, tol = ref[:, 4:], tol[:, 4:]
    tol16 = R.fp16_store_tol(ref, tol)

    def run(v, out):
        return L.rva_conv1x1_head_f16(ctx.handle, _ptr(x), 128, _ptr(wt), _ptr(bias), B, h, w, 128, nc, 2, _ptr(out), nc, A, R.A0,
                                      C.c_float(stride), v, s)
    probe = _fill((B, 4 + nc, A), torch.float16)
    bad = []
    for v in _accepted(lambda v: run(v, probe)):
        what = f"{R.geometry_id(geometry)} variant {v}"
        out = _fill((B, 4 + nc, A), torch.float16)
        ctx.check(run(v, out), "rva_conv1x1_head_f16")
        torch.cuda.synchronize()
        R.check("rva_conv1x1_head_f16 mode 2 scores", what, _level(out, R.A0, hw, what, slice(4, 4 + nc)), ref, tol16, bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ refused calls
def test_bad_head_arguments_are_refused_before_any_launch():
    """Each bad call returns RVA_ERR_ARG and leaves the sentinel-filled output untouched.  The output is allocated for 2 A anchors
    while the calls declare A: a library without the anchor-range check would still write inside the allocation, so this test can
    only fail by the return code and the sentinel, never by a fault."""
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, h, w, nc = 2, 20, 13, 8
    hw = h * w
    A = hw + R.PAD_ANCHORS
    box = torch.zeros((B, h, w, 144), dtype=torch.float16, device="cuda")      # wide enough for every ld tried below
    cls = torch.zeros((B, h, w, 144), dtype=torch.float16, device="cuda")
    out = _fill((B, 4 + 16, 2 * A), torch.float16)
    b32 = _fill((B, 4, 2 * A), torch.float32)
    good = dict(ldb=64, ldc=8, batch=B, h=h, w=w, nc=nc, A=A, a0=R.A0)

    def head(**kw):
        a = {**good, **kw}
        return L.rva_yolo_head_f16(ctx.handle, _ptr(box), a["ldb"], _ptr(cls), a["ldc"], _ptr(out), a["batch"], a["h"], a["w"], a["nc"],
                                   a["A"], a["a0"], C.c_float(8.0), s)

    def head_box32(**kw):
        a = {**good, **kw}
        return L.rva_yolo_head_box32_f16(ctx.handle, _ptr(box), a["ldb"], _ptr(cls), a["ldc"], _ptr(out), _ptr(b32), a["batch"], a["h"],
                                         a["w"], a["nc"], a["A"], a["a0"], C.c_float(8.0), s)
    bad_calls = [dict(batch=0), dict(batch=-1), dict(h=0), dict(w=0), dict(h=-h), dict(a0=-1), dict(a0=A - hw + 1), dict(A=hw - 1, a0=0),
                 dict(nc=4), dict(nc=12), dict(ldb=68), dict(ldc=12)]
    for fn in (head, head_box32):
        for kw in bad_calls:
            assert fn(**kw) == N.RVA_ERR_ARG, (fn.__name__, kw)
    # three levels whose anchors do not add up to anchors_total (one too few, one too many), and a bad level
    levels = R.HEAD3_CASES[0]
    A3 = sum(a * b for a, b in levels)
    assert A3 + 1 <= 2 * A
    ptrs, _k1 = N.ptr_array([box.data_ptr()] * 3)
    cptrs, _k2 = N.ptr_array([cls.data_ptr()] * 3)
    ld, _k3 = N.i32_array([64] * 3)
    ldc, _k4 = N.i32_array([8] * 3)
    ldc_bad, _k5 = N.i32_array([8, 12, 8])
    hp, _k6 = N.i32_array([a for a, _ in levels])
    wp, _k7 = N.i32_array([b for _, b in levels])
    sp = (C.c_float * 3)(*R.STRIDES)
    for total, ldcs, ncs in ((A3 - 1, ldc, nc), (A3 + 1, ldc, nc), (A3, ldc_bad, nc), (A3, ldc, 12)):
        assert L.rva_yolo_head3_f16(ctx.handle, ptrs, ld, cptrs, ldcs, _ptr(out), 1, hp, wp, ncs, total, sp, s) == N.RVA_ERR_ARG
        assert L.rva_yolo_head3_box32_f16(ctx.handle, ptrs, ld, cptrs, ldcs, _ptr(out), _ptr(b32), 1, hp, wp, ncs, total, sp, s) == N.RVA_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((b32 == SENTINEL).all())
    # and the good call is accepted and writes the level alone
    ctx.check(head(), "rva_yolo_head_f16")
    torch.cuda.synchronize()
    flat = out.flatten().cpu()
    used = flat[:B * (4 + nc) * A].view(B, 4 + nc, A)                         # the tensor the call declared
    assert bool((used[:, :, R.A0:R.A0 + hw] != SENTINEL).all()) and bool((flat[B * (4 + nc) * A:] == SENTINEL).all())
    assert bool((used[:, :, :R.A0] == SENTINEL).all()) and bool((used[:, :, R.A0 + hw:] == SENTINEL).all())
