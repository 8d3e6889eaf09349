"""Every row of the fp16 convolution variant table (``kConvVariants``, csrc/rva_conv.hip) where the fused plan really calls
it: on channel slices of concat buffers with the plan's row strides, offsets and rounded-up Cin (part 1, against float64), and
forced on the steps of real plans (part 2: YOLOv8 plans against the rounding-matched reference, YOLOv5 and YOLO11 plans against
the float64 module with PyTorch fp16's error as the yardstick).  The autotuner picks rows by time alone; these tests are what
makes "all variants compute the same layer" true for the layouts it picks them on.  ``FusedYoloV5`` and ``FusedYolo11`` inherit
the tuner unchanged, and their builders produce layouts the YOLOv8 builder never does -- ``Builder::c3`` / ``build_v5``:
residuals in another allocation, cv3 from the middle of a row; ``Builder::build_11`` / ``c2psa``: 8-channel buffers, bottlenecks
with Cin != Cout, a C3k nested in a slice of a C2f row, a residual without activation, a zero-extended class branch.  Both parts
cover all three builders."""
import collections
import ctypes as C
import copy
import functools
import gc
import json
import os
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.engine import FusedYolo11, FusedYoloV5, FusedYoloV8
from realtime_video_analytics_32streams_amd.yolo11 import build_detector_net_11
from realtime_video_analytics_32streams_amd.yolov5 import build_detector_net_v5
from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net
from tests.conv_slice_layouts import (Layout, V5_STRIDE1_LAYOUTS, V5_STRIDE2_LAYOUTS, V11_STRIDE1_LAYOUTS, V11_STRIDE2_LAYOUTS,
                                      zero_extend)
from tests.helpers import (V5_GROUPS, V11_GROUPS, assert_conv_close, assert_matches_rounded_reference, plan_rounded_reference, v5_head_errors,
                           v5_groups_over_twice_torch)

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


# ---------------------------------------------------------------------------------------------------
# Part 1: rva_conv2d_nhwc_f16_v on the plan's slice layouts
# ---------------------------------------------------------------------------------------------------
def _cv1(c, decl, n, i):
    """Bottleneck cv1: reads cat.sub((1+i)*c, c) of a (2+n)*c row, writes the contiguous tmp."""
    return Layout(f"cv1 c{c} n{n} i{i}", c, decl, c, 3, 1, 1, ((2 + n) * c, (1 + i) * c), (c, 0))


def _cv2(c, decl, n, i, shortcut=True):
    """Bottleneck cv2: reads the contiguous tmp, writes cat.sub((2+i)*c, c); the shortcut is the neighbouring slice."""
    ld = (2 + n) * c
    return Layout(f"cv2 c{c} n{n} i{i}" + ("" if shortcut else " no shortcut"), c, decl, c, 3, 1, 1, (c, 0), (ld, (2 + i) * c),
                  (ld, (1 + i) * c) if shortcut else None)


STRIDE1_LAYOUTS = [
    # Builder::c2f / Builder::bottleneck (`conv1(b1, x, tmp, ...)` with x = cat.sub((1+i)*c, c)).
    _cv1(16, 32, 1, 0),        # YOLOv8n b2: Cin 16 declared 32; the 16 channels read past the slice are the row's last slice
    _cv1(16, 32, 2, 0),        # ... are a real neighbour in the middle of the row
    _cv1(48, 64, 1, 0),        # YOLOv8m b2 widths: Cin 48 declared 64, past = last slice
    _cv1(48, 64, 2, 0),        # ... past = the neighbour slice
    _cv1(48, 64, 2, 1),        # ... past = the last slice, behind two slices
    _cv1(64, 64, 2, 1),        # YOLOv8n b6 / s b4: nothing read past the slice
    _cv1(128, 128, 1, 0),      # YOLOv8n b8 / s b6
    # Builder::c2f / Builder::bottleneck (`conv1(b2, tmp, y, ..., shortcut ? &x : nullptr)` with y = cat.sub((2+i)*c, c)): contiguous tmp in --
    # with c = 16 / 48 the declared Cin reaches into the next pixel and, behind the last pixel, into the 64-byte slack --
    # output slice and residual slice side by side in one allocation, ldr = ldo = (2+n)*c
    _cv2(16, 32, 1, 0),
    _cv2(48, 64, 2, 1),
    _cv2(64, 64, 2, 0),
    _cv2(128, 128, 1, 0),
    _cv2(32, 32, 1, 0, shortcut=False),        # neck C2f (h15 of YOLOv8n): no shortcut
    # Builder::c2f / Builder::build (C2f closing 1x1 `conv1(cv2, cat, dst, ...)` with dst = p3 = cat15.sub(c4, c3)): whole cat row in, back
    # half of a neck concat buffer out, ldo = c4 + c3 and offset c4 (YOLOv8n b4: c = 32, n = 2)
    Layout("c2f close -> p3", 128, 128, 64, 1, 1, 1, (128, 0), (128 + 64, 128)),
    # Builder::c2f (the same of YOLOv8n b2: cat of 3 x 16 channels declared 64, read into the next pixel / the slack)
    Layout("c2f close c16", 48, 64, 32, 1, 1, 1, (48, 0), (32, 0)),
    # Builder::build (`conv1(hd.box[l][1], first.sub(0, cb), b2, ...)`): row stride cb + cc = 144 halves = 288 bytes (YOLOv8n)
    Layout("detect box.1 n", 64, 64, 64, 3, 1, 1, (64 + 80, 0), (64, 0)),
    # Builder::build (`conv1(cls[l][1], first.sub(cb, cc), k2, ...)`).  YOLOv8n: cc = 80 declared 96, so the step reads 16
    # channels of the NEXT pixel's box half; YOLOv8s: cc = 128, row stride 192
    Layout("detect cls.1 n", 80, 96, 80, 3, 1, 1, (64 + 80, 64), (80, 0)),
    Layout("detect cls.1 s", 128, 128, 128, 3, 1, 1, (64 + 128, 64), (128, 0)),
    # Builder::head_last (`conv1(c, src, o, l, 0)`, the unfused head of YOLOv8n): no activation, Cin 80 declared 96 on a
    # contiguous 80-channel buffer
    Layout("detect cls.2 n", 80, 96, 80, 1, 1, 0, (80, 0), (80, 0)),
    # Builder::build (sibling launch `conv(sib, 2, feats[l], first, ...)`): Cout = cb + cc = 144 across the 64- and 96-channel tiles
    Layout("detect first n", 64, 64, 64 + 80, 3, 1, 1, (64, 0), (64 + 80, 0)),
]

STRIDE2_LAYOUTS = [
    # Builder::backbone (`conv1(take(x.ch, t.ch, 3, 2, "b5"), x, t, ...)`, x = p3 = cat15.sub(c4, c3)): reads a back-half slice
    Layout("b5 n", 64, 64, 128, 3, 2, 1, (128 + 64, 128), (128, 0)),
    Layout("b5 m", 192, 192, 384, 3, 2, 1, (384 + 192, 384), (384, 0)),
    # Builder::bottom_up (`conv1(take(x.ch, x.ch, 3, 2, "h16"), x, cat[i].sub(0, x.ch), ...)`, x = n3, cat18): writes a front-half slice
    Layout("h16 n", 64, 64, 64, 3, 2, 1, (64, 0), (64 + 128, 0)),
    # Builder::backbone (`b3` of YOLOv8n, 32 -> 64: the Cin = 32 stride-2 patch kernel) into a front-half slice as h16 writes it
    Layout("s2 32->64 front half", 32, 32, 64, 3, 2, 1, (32, 0), (64 + 128, 0)),
]

# The YOLOv5 builder (Builder::c3 and Builder::build_v5): residuals in another allocation with ldr != ldo, sibling launches into
# the front of a 3c row, cv3 from its middle, padded Cin under a stride-2 3x3.  Generated from a restatement of the builder
# (tests/conv_slice_layouts.py, which cites the statement of each step), not typed by hand.
STRIDE1_LAYOUTS += V5_STRIDE1_LAYOUTS
STRIDE2_LAYOUTS += V5_STRIDE2_LAYOUTS

# The YOLO11 builder (Builder::build_11 through Builder::c2f, Builder::bottleneck with cmid = c / 2, Builder::c3 with k1 = 3, and
# Builder::c2psa): Cout = 8 and Cin = 8 declared 32 on a 16-byte row, bottlenecks with Cin != Cout on concat slices, a C3k nested in
# a slice of the outer row, act = 0 with a residual (ldr = ldo and ldr != ldo), cv1 of C2PSA as two launches, the class branch's
# zero-extended pointwise convolutions.  Generated like the YOLOv5 ones; build_11 has no stride-2 step of a new kind.
STRIDE1_LAYOUTS += V11_STRIDE1_LAYOUTS
STRIDE2_LAYOUTS += V11_STRIDE2_LAYOUTS

# B, H, W: tiles that straddle rows and images, and an M tail (9 x 7: 189 pixels); stride 2 with even sizes (the s2run rows)
STRIDE1_SHAPES = [(3, 12, 20), (3, 6, 10), (3, 9, 7)]
STRIDE2_SHAPES = [(2, 12, 20)]
CASES = [(lay, s) for lay in STRIDE1_LAYOUTS for s in STRIDE1_SHAPES] + [(lay, s) for lay in STRIDE2_LAYOUTS for s in STRIDE2_SHAPES]


def _plan_buffer(m, ld, fill):
    """An activation buffer as ``Builder::buf()`` allocates it: exactly ``m * ld`` halves and 64 bytes of zero slack."""
    t = torch.zeros((m * ld * 2 + 64,), dtype=torch.uint8, device="cuda").view(torch.float16)
    t[:m * ld] = fill.reshape(-1).to(device="cuda", dtype=torch.float16)
    return t


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("layout,shape", CASES, ids=[f"{lay.name} {b}x{h}x{w}".replace(" ", "_") for lay, (b, h, w) in CASES])
def test_every_variant_on_a_plan_slice_matches_float64(layout, shape):
    """Each row of the variant table on one slice layout of the plan: within the fp16-ulp bound of the float64 convolution of the
    real channels, nothing written outside the output slice (nor into a residual buffer of its own), nothing taken from outside the
    declared input slice, and the same rows accepted as for the contiguous tensor of that shape."""
    lay, (B, H, W) = layout, shape
    k, s = lay.k, lay.stride
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    Mi, Mo = B * H * W, B * Ho * Wo
    (ldi, offi), (ldo, offo) = lay.inp, lay.out
    assert offi % 8 == 0 and offo % 8 == 0 and offi + lay.cin <= ldi and offo + lay.cout <= ldo
    g = torch.Generator().manual_seed(11)
    x_rows = (torch.randn((Mi, ldi), generator=g) * 0.5).half()
    w = (torch.randn((lay.cout, lay.cin, k, k), generator=g) / (lay.cin * k * k) ** 0.5).half()
    b = torch.randn((lay.cout,), generator=g) * 0.1
    w, b = zero_extend(lay, w, b)             # the class branch of YOLO11: zero past the checkpoint's channels, as Builder::padded
    out_rows = torch.full((Mo, ldo), SENTINEL, dtype=torch.float16)
    res, res_init, ldr = None, None, 0
    if lay.res is not None:
        ldr, offr = lay.res
        assert offr % 8 == 0 and offr + lay.cout <= ldr
        if lay.res_own:                   # a buffer of its own, every channel of its rows random: row stride and offset are its own
            res_rows = (torch.randn((Mo, ldr), generator=g) * 0.5).half()
            res = res_rows[:, offr:offr + lay.cout].contiguous()
            res_init = _plan_buffer(Mo, ldr, res_rows)
        else:                             # a neighbouring slice of the output rows
            assert ldr == ldo and (offr + lay.cout <= offo or offr >= offo + lay.cout)
            res = (torch.randn((Mo, lay.cout), generator=g) * 0.5).half()
            out_rows[:, offr:offr + lay.cout] = res

    # float64 reference on the fp16-rounded operands: the real Cin channels and the real Cout rows only
    xs = x_rows[:, offi:offi + lay.cin].reshape(B, H, W, lay.cin).double().permute(0, 3, 1, 2)
    y = F.conv2d(xs, w.double(), b.double(), stride=s, padding=k // 2)
    if lay.act:
        y = y * torch.sigmoid(y)
    want = y.permute(0, 2, 3, 1).reshape(Mo, lay.cout)
    if res is not None:
        want = want + res.double()
    want = want.cuda()
    res_dev = res.cuda() if res is not None else None

    L, ctx = N.lib(), ops.context()
    cpad, cinp = L.rva_conv_cout_pad(lay.cout), (lay.cin_decl + 31) // 32 * 32
    wp = torch.zeros((cpad, k * k, cinp), dtype=torch.float16)
    wp[:lay.cout, :, :lay.cin] = w.permute(0, 2, 3, 1).reshape(lay.cout, k * k, lay.cin)      # columns cin.. stay zero, as Builder::pack
    bp = torch.zeros(cpad)
    bp[:lay.cout] = b
    wp, bp = wp.cuda(), bp.cuda()

    x_buf = _plan_buffer(Mi, ldi, x_rows)
    # the same slice with everything else of every row replaced: what the zero weight columns (and nothing else) may touch
    other = x_rows.clone()
    outside = torch.ones(ldi, dtype=torch.bool)
    outside[offi:offi + lay.cin] = False
    sign = torch.where(torch.arange(Mi * ldi).reshape(Mi, ldi) % 2 == 0, 6.0e4, -6.0e4).half()
    other[:, outside] = sign[:, outside]
    x_other = _plan_buffer(Mi, ldi, other) if bool(outside.any()) else None
    out_init = _plan_buffer(Mo, ldo, out_rows)
    written = torch.zeros((Mo, ldo), dtype=torch.bool)
    written[:, offo:offo + lay.cout] = True
    untouched = torch.cat((~written.reshape(-1), torch.ones(32, dtype=torch.bool))).cuda()      # the rest of the rows + the slack
    # the contiguous call of the same shape (declared Cin, ld = C, offset 0): decides nothing but which rows apply
    xc = _plan_buffer(Mi, lay.cin_decl, torch.randn((Mi, lay.cin_decl), generator=g) * 0.5)
    oc = _plan_buffer(Mo, lay.cout, torch.zeros((Mo, lay.cout)))
    rc_res = _plan_buffer(Mo, lay.cout, res) if res is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(variant, xin, ld_in, off_in, out, ld_out, off_out, resid, ld_res):
        return L.rva_conv2d_nhwc_f16_v(ctx.handle, C.c_void_p(xin.data_ptr() + 2 * off_in), ld_in, C.c_void_p(wp.data_ptr()),
                                       C.c_void_p(bp.data_ptr()), C.c_void_p(out.data_ptr() + 2 * off_out), ld_out,
                                       C.c_void_p(resid) if resid else None, ld_res, B, H, W, lay.cin_decl, lay.cout, k, s, lay.act,
                                       variant, stream)

    res_buf = res_init.clone() if res_init is not None else None

    def residual_of(out):
        """Address of the residual slice for a launch that writes ``out``: in ``out`` itself, or in the separate buffer."""
        if lay.res is None:
            return 0
        return (res_buf if lay.res_own else out).data_ptr() + 2 * lay.res[1]

    on_slice, on_contiguous = [], []
    for v in range(0, L.rva_conv_num_variants() + 1):
        name = (v, (L.rva_conv_variant_name(v) or b"?").decode())
        out = out_init.clone()
        resid = residual_of(out)
        rc = launch(v, x_buf, ldi, offi, out, ldo, offo, resid, ldr if resid else 0)
        if rc != N.RVA_ERR_ARG:
            assert rc == N.RVA_OK, (name, rc)
            torch.cuda.synchronize()                 # a HIP error ends the test here: nothing more is launched after it
            on_slice.append(v)
            got = out[:Mo * ldo].reshape(Mo, ldo)[:, offo:offo + lay.cout].double()
            # a residual without activation (Builder::c2psa) is rounded like one behind SiLU: conv + bias to fp16, the sum in
            # fp32, to fp16 again, and the first rounded value is at most |want| + |res|: the bound's `res` term holds as it is
            assert_conv_close(got, want, res_dev, name)
            assert torch.equal(_bits(out)[untouched], _bits(out_init)[untouched]), (name, "wrote outside its output slice")
            if res_buf is not None:
                assert torch.equal(_bits(res_buf), _bits(res_init)), (name, "wrote to the residual buffer")
            if x_other is not None:
                out2 = out_init.clone()
                resid2 = residual_of(out2)
                rc = launch(v, x_other, ldi, offi, out2, ldo, offo, resid2, ldr if resid2 else 0)
                assert rc == N.RVA_OK, (name, rc)
                torch.cuda.synchronize()
                assert torch.equal(_bits(out2), _bits(out)), (name, "result depends on channels outside the declared slice")
        rc = launch(v, xc, lay.cin_decl, 0, oc, lay.cout, 0, rc_res.data_ptr() if rc_res is not None else 0, lay.cout if rc_res is not None else 0)
        if rc != N.RVA_ERR_ARG:
            assert rc == N.RVA_OK, (name, "contiguous", rc)
            torch.cuda.synchronize()
            on_contiguous.append(v)
    print(f"[{lay.name} {B}x{H}x{W}] rows that applied: {len(on_slice)}")
    assert 0 in on_slice and len(on_slice) >= 3, on_slice
    assert on_slice == on_contiguous, ("applicability depends on strides", sorted(set(on_slice) ^ set(on_contiguous)))


# ---------------------------------------------------------------------------------------------------
# Part 2: every row forced on the steps of real plans
# ---------------------------------------------------------------------------------------------------
# scale, batch, (H, W), environment at construction.  (96, 160): levels 12 x 20, 6 x 10, 3 x 5 -- even where a step upsamples -- and
# batch 3 so that tiles straddle images; 640 x 640 at batch 1 puts the W <= 160 and 2^24 gates where production has them.
# RVA_PAIR32=0 turns the fused 32 -> 32 bottleneck pairs into convolution steps, RVA_NO_STEM2=1 the first downsampling convolution.
CONFIGS = {
    "n": ("n", 3, (96, 160), {}),
    "s": ("s", 3, (96, 160), {}),
    "m": ("m", 3, (96, 160), {}),
    "s-640": ("s", 1, (640, 640), {}),
    "s-no-pair32": ("s", 3, (96, 160), {"RVA_PAIR32": "0"}),
    "s-no-stem2": ("s", 3, (96, 160), {"RVA_NO_STEM2": "1"}),
}
_PLAN_ENV = ("RVA_PAIR32", "RVA_NO_STEM2", "RVA_NO_CIN_PAD", "RVA_TUNE_LAYER_OVERLAP", "RVA_SERIAL_HEADS")

# Rows that no convolution step of any configuration above accepts, with the launcher's gate that keeps them out.
NEVER_APPLIES = {}

_forced = {}           # configuration -> [(desc, variant)] or the exception that ended it (never run twice)


def _once(key, run):
    """``run()`` for configuration ``key``, once per session: a configuration that failed is never run again."""
    if key in _forced:
        if isinstance(_forced[key], BaseException):
            pytest.fail(f"configuration {key} failed earlier in this session: {_forced[key]!r}")
        return _forced[key]
    try:
        _forced[key] = run()
    except BaseException as exc:
        _forced[key] = exc
        raise
    return _forced[key]


def _force_every_variant(key, monkeypatch):
    def run():
        scale, batch, hw, env = CONFIGS[key]
        with monkeypatch.context() as mp:
            for name in _PLAN_ENV:
                mp.delenv(name, raising=False)
            for name, value in env.items():
                mp.setenv(name, value)
            net = build_detector_net(scale, seed=3)
            plan = FusedYoloV8(net, batch, hw=hw, autotune=False)      # the tuning cache is not consulted
        x = torch.rand((batch, 3, *hw), device="cuda", generator=torch.Generator(device="cuda").manual_seed(17)).half()
        want = plan_rounded_reference(net, x)
        return _run_forced(plan, x, lambda got: assert_matches_rounded_reference(got, want))
    return _once(key, run)


def _run_forced(plan, x, check):
    """``check(got)`` raises AssertionError where the head tensor misses the configuration's condition; what it returns is printed."""
    L = N.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run_and_check(what):
        got = plan(x)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got).all()), (what, "non-finite output")
        try:
            return check(got)
        except AssertionError as exc:
            raise AssertionError((what, *exc.args)) from None

    assert all(state["variant"] == 0 for _, state, _ in plan._tunable)
    print("variant 0:", run_and_check("variant 0"))
    ran = []
    try:
        for v in range(1, L.rva_conv_num_variants() + 1):
            picks = []
            for launch, _, desc in plan._tunable:
                rc = launch(stream, v)                   # the autotuner's probe: RVA_ERR_ARG = "does not apply", from host code
                assert rc in (N.RVA_OK, N.RVA_ERR_ARG), (desc, v, rc)
                picks.append(v if rc == N.RVA_OK else 0)
            torch.cuda.synchronize()
            if not any(picks):
                continue
            for (_, state, _), pv in zip(plan._tunable, picks):
                state["variant"] = pv
            try:
                run_and_check(("variant", v))
            except AssertionError as exc:
                # name the steps: one at a time (a HIP error is no AssertionError and ends everything above)
                guilty = []
                for i, (_, state, desc) in enumerate(plan._tunable):
                    if not picks[i]:
                        continue
                    for j, (_, other, _) in enumerate(plan._tunable):
                        other["variant"] = v if j == i else 0
                    try:
                        run_and_check(desc)
                    except AssertionError as one:
                        guilty.append((desc, one.args))
                raise AssertionError((exc.args, "steps that miss alone", guilty)) from None
            ran += [(desc, v) for (_, _, desc), pv in zip(plan._tunable, picks) if pv]
    finally:
        for _, state, _ in plan._tunable:
            state["variant"] = 0
    return ran


@pytest.mark.parametrize("key", list(CONFIGS))
def test_every_variant_forced_on_the_plan_steps(key, monkeypatch):
    """Variant v on every step that accepts it (0 on the rest), for every v: the whole plan stays within the project's bound of
    the rounding-matched reference (``assert_matches_rounded_reference`` at its defaults), as with variant 0."""
    ran = _force_every_variant(key, monkeypatch)
    print(f"{key}: {len(ran)} (step, variant) pairs forced, {len({v for _, v in ran})} distinct rows")
    assert ran


def test_forced_variants_cover_the_table(monkeypatch):
    """Over all configurations every row ran on a real plan step, but for the rows listed in NEVER_APPLIES; each LDS-DMA gather
    tile (33..39) ran on an upsample + concat step and on a fused head step of each mode."""
    ran = [pair for key in CONFIGS for pair in _force_every_variant(key, monkeypatch)]
    rows = set(range(1, N.lib().rva_conv_num_variants() + 1))
    seen = {v for _, v in ran}
    assert rows - seen == set(NEVER_APPLIES), sorted(rows - seen)
    for v in range(33, 40):
        for prefix in ("up", "head1:", "head2:"):
            assert any(pv == v and desc.startswith(prefix) for desc, pv in ran), (v, prefix)


# ---------------------------------------------------------------------------------------------------
# Part 2 for the YOLOv5 builder: every row forced on the steps of real YOLOv5 plans
# ---------------------------------------------------------------------------------------------------
# scale, batch, (H, W).  Scale m is where c = 48 brings the padded Cin and the two-bottleneck neck blocks; 640 x 640 as above.
V5_CONFIGS = {
    "v5n": ("n", 3, (96, 160)),
    "v5s": ("s", 3, (96, 160)),
    "v5m": ("m", 3, (96, 160)),
    "v5s-640": ("s", 1, (640, 640)),
}

# Rows that no convolution step of any YOLOv5 configuration above accepts, with the launcher's gate that keeps them out.
NEVER_APPLIES_V5 = {}

_v5_errors = {}        # configuration -> what is recorded as profiles/yolov5_variants.json


@functools.lru_cache(maxsize=None)
def _v5_net(scale):
    """Seeded, BatchNorm folded, every parameter rounded to fp16 (kept as fp32), as ``_net()`` of tests/test_gpu_yolov5_plan.py:
    the plan, the fp16 module and the float64 module hold the same numbers.  Shared, never modified."""
    net = build_detector_net_v5(scale, seed=3).fuse()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.half().float())
    return net


def _record_variants(fname, key, value):
    out = os.environ.get("RVA_REPORT_DIR")
    if out and Path(out).is_dir():
        path = Path(out) / fname
        data = json.loads(path.read_text()) if path.exists() else {}
        data[key] = value
        path.write_text(json.dumps(data, indent=1, sort_keys=True))


def _forced_against_float64(key, plan, net, x, head, groups):
    """Every row forced on ``plan`` (``_run_forced``) under the yardstick of the fp16 plans: per row group of ``groups`` at most
    twice the error of the same module in PyTorch fp16 channels-last, both against the float64 module on the CPU; variant 0 is held
    to it first.  ``head`` turns the module's output into the plan's ``[B, rows, A]``.  Returns the forced pairs and, per group, the
    errors of variant 0, of PyTorch, the largest error of any forced run and the row that gave it."""
    with torch.inference_mode():
        want = head(copy.deepcopy(net).double()(x.double())).contiguous().cuda()
        ref16 = copy.deepcopy(net).half().cuda().to(memory_format=torch.channels_last)
        tor = head(ref16(x.cuda().contiguous(memory_format=torch.channels_last))).double()
    x = x.cuda()
    rec = {}

    def check(got):
        errs = v5_head_errors(got.double(), tor, want, groups)
        for name, e in errs.items():
            r = rec.setdefault(name, {"variant0_max_err": e["plan_max_err"], "torch_fp16_max_err": e["torch_fp16_max_err"],
                                      "forced_max_err": 0.0, "forced_max_err_row": 0})
            row = max((st["variant"] for _, st, _ in plan._tunable), default=0)
            if row and e["plan_max_err"] > r["forced_max_err"]:
                r["forced_max_err"], r["forced_max_err_row"] = e["plan_max_err"], row
        bad = v5_groups_over_twice_torch(errs)
        assert not bad, ("plan error over twice PyTorch fp16's (group, plan, PyTorch)", bad)
        return {name: (e["plan_max_err"], e["torch_fp16_max_err"]) for name, e in errs.items()}
    try:
        ran = _run_forced(plan, x, check)
    finally:
        for name, r in rec.items():
            print(f"[{key}] {name}: variant 0 max |d| {r['variant0_max_err']:.4g}, forced rows max |d| {r['forced_max_err']:.4g} "
                  f"(row {r['forced_max_err_row']}), PyTorch fp16 max |d| {r['torch_fp16_max_err']:.4g}")
    return ran, rec


def _force_every_variant_v5(key, monkeypatch):
    """The yardstick is the plan's own (tests/test_gpu_yolov5_plan.py), see ``_forced_against_float64``."""
    def run():
        scale, batch, hw = V5_CONFIGS[key]
        net = _v5_net(scale)
        with monkeypatch.context() as mp:
            for name in _PLAN_ENV:
                mp.delenv(name, raising=False)
            plan = FusedYoloV5(copy.deepcopy(net), batch, hw=hw, autotune=False)      # the tuning cache is not consulted
        x = torch.rand((batch, 3, *hw), generator=torch.Generator().manual_seed(17)).half()
        ran, rec = _forced_against_float64(key, plan, net, x, lambda t: t.transpose(1, 2), V5_GROUPS)
        _v5_errors[key] = {"scale": scale, "batch": batch, "hw": list(hw), "step_variant_pairs": len(ran),
                           "distinct_rows": len({v for _, v in ran}), "groups": rec}
        _record_variants("yolov5_variants.json", key, _v5_errors[key])
        return ran
    return _once(key, run)


@pytest.mark.parametrize("key", list(V5_CONFIGS))
def test_every_variant_forced_on_the_yolov5_plan_steps(key, monkeypatch):
    """Variant v on every step of a YOLOv5 plan that accepts it (0 on the rest), for every v: each row group of the head tensor
    stays within twice PyTorch fp16's error against the float64 module, as variant 0 must; non-finite output fails."""
    ran = _force_every_variant_v5(key, monkeypatch)
    print(f"{key}: {len(ran)} (step, variant) pairs forced, {len({v for _, v in ran})} distinct rows")
    assert ran


def test_forced_variants_cover_the_table_on_yolov5(monkeypatch):
    """Over the YOLOv5 configurations every row ran on a real plan step, but for the rows listed in NEVER_APPLIES_V5; each
    LDS-DMA gather tile (33..39) ran on an upsample + concat step and on a fused head step."""
    per_key = {key: _force_every_variant_v5(key, monkeypatch) for key in V5_CONFIGS}
    for key, ran in per_key.items():
        print(f"{key}: {len(ran)} (step, variant) pairs")
    ran = [pair for pairs in per_key.values() for pair in pairs]
    rows = set(range(1, N.lib().rva_conv_num_variants() + 1))
    seen = {v for _, v in ran}
    assert rows - seen == set(NEVER_APPLIES_V5), sorted(rows - seen)
    for v in range(33, 40):
        for prefix in ("up", "head5:"):
            assert any(pv == v and desc.startswith(prefix) for desc, pv in ran), (v, prefix)


# ---------------------------------------------------------------------------------------------------
# Part 2 for the YOLO11 builder: every row forced on the steps of real YOLO11 plans
# ---------------------------------------------------------------------------------------------------
# scale, classes, batch, (H, W).  n has the 8-channel steps (`2`: 16 -> 8 -> 16) and an unfused head, s and m the fused head steps,
# m and l a C3k in every C3k2 (widths 64 to 512), l two inner blocks per C3k2 and two PSA blocks; nc 85 pads the class branch to 88
# with zero-extended weights; 640 x 640 at batch 1 puts the W <= 160 and 2^24 gates where production has them (400 tokens in C2PSA).
V11_CONFIGS = {
    "11n": ("n", 80, 3, (96, 160)),
    "11s": ("s", 80, 3, (96, 160)),
    "11m": ("m", 80, 3, (96, 160)),
    "11n-nc85": ("n", 85, 3, (96, 160)),
    "11n-640": ("n", 80, 1, (640, 640)),
    "11l": ("l", 80, 1, (96, 160)),
}

# Rows that no convolution step of any YOLO11 configuration above accepts, with the launcher's gate that keeps them out.
NEVER_APPLIES_11 = {}

_v11_errors = {}       # configuration -> what is recorded as profiles/yolo11_variants.json


@functools.lru_cache(maxsize=None)
def _v11_net(scale, nc):
    """Seeded, BatchNorm folded, every parameter rounded to fp16 (kept as fp32), as ``_net()`` of tests/test_gpu_yolo11_plan.py.
    Shared, never modified."""
    net = build_detector_net_11(scale, seed=7, nc=nc).fuse()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.half().float())
    return net


def _force_every_variant_11(key, monkeypatch):
    """The yardstick is the plan's own (tests/test_gpu_yolo11_plan.py), see ``_forced_against_float64``."""
    def run():
        scale, nc, batch, hw = V11_CONFIGS[key]
        net = _v11_net(scale, nc)
        with monkeypatch.context() as mp:
            for name in _PLAN_ENV:
                mp.delenv(name, raising=False)
            plan = FusedYolo11(copy.deepcopy(net), batch, hw, autotune=False)         # the tuning cache is not consulted
        x = torch.rand((batch, 3, *hw), generator=torch.Generator().manual_seed(17)).half()
        ran, rec = _forced_against_float64(key, plan, net, x, lambda t: t, V11_GROUPS)
        _v11_errors[key] = {"scale": scale, "nc": nc, "batch": batch, "hw": list(hw), "step_variant_pairs": len(ran),
                            "distinct_rows": len({v for _, v in ran}), "groups": rec}
        _record_variants("yolo11_variants.json", key, _v11_errors[key])
        del plan
        gc.collect()          # a plan is in a reference cycle with its tunables: free its device buffers now, not in some later test
        return ran
    return _once(key, run)


@pytest.mark.parametrize("key", list(V11_CONFIGS))
def test_every_variant_forced_on_the_yolo11_plan_steps(key, monkeypatch):
    """Variant v on every step of a YOLO11 plan that accepts it (0 on the rest), for every v: each row group of the head tensor
    (boxes, classes) stays within twice PyTorch fp16's error against the float64 module, as variant 0 must; non-finite output
    fails."""
    ran = _force_every_variant_11(key, monkeypatch)
    print(f"{key}: {len(ran)} (step, variant) pairs forced, {len({v for _, v in ran})} distinct rows")
    assert ran


def test_forced_variants_cover_the_table_on_yolo11(monkeypatch):
    """Over the YOLO11 configurations every row ran on a real plan step, but for the rows listed in NEVER_APPLIES_11; each LDS-DMA
    gather tile (33..39) ran on an upsample + concat step and on a fused head step of each mode; and the steps only this builder
    produces were among the forced pairs of YOLO11n: the 8-channel bottleneck, the 3x3 -> 3x3 bottlenecks of the nested C3k, and a
    1x1 without activation.  A description does not carry the activation: ``128->256 k1s1`` at stride 32 is qkv (none) and ffn.0
    (SiLU) of ``Builder::c2psa`` and nothing else, so a row forced on two steps of that description ran on qkv."""
    per_key = {key: _force_every_variant_11(key, monkeypatch) for key in V11_CONFIGS}
    for key, ran in per_key.items():
        print(f"{key}: {len(ran)} (step, variant) pairs")
    ran = [pair for pairs in per_key.values() for pair in pairs]
    rows = set(range(1, N.lib().rva_conv_num_variants() + 1))
    seen = {v for _, v in ran}
    assert rows - seen == set(NEVER_APPLIES_11), sorted(rows - seen)
    for v in range(33, 40):
        for prefix in ("up", "head1:", "head2:"):
            assert any(pv == v and desc.startswith(prefix) for desc, pv in ran), (v, prefix)
    pairs = collections.Counter((desc.split(" r[")[0], v) for desc, v in per_key["11n"])
    forced_on = {desc for desc, _ in pairs}
    h5, w5 = 96 // 32, 160 // 32
    for desc in (f"16->8 k3s1 {8 * h5}x{8 * w5}", f"8->16 k3s1 {8 * h5}x{8 * w5}", f"64->64 k3s1 {h5}x{w5}", f"128->256 k1s1 {h5}x{w5}"):
        assert desc in forced_on, (desc, sorted(forced_on))
    assert max(n for (desc, _), n in pairs.items() if desc == f"128->256 k1s1 {h5}x{w5}") == 2
