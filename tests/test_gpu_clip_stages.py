"""Every stage of the fp32 CNN-LSTM clip plan (csrc/rva_clip.hip) against float64 on the GPU, through the read-only workspace
tap ``rva_cnnlstm_plan_stage``: the stem's pooled map, conv2's tile partials, the spatial mean, layer 1's input projection,
both LSTM layers at every step and clip, and the logits.  Each stage's reference is computed from the tap of the stage before
it with the bounds of tests/clip_stage_refs.py, so a failure names the kernel; tests/test_clip_stages_host.py proves on the
CPU that these bounds see the kernels' bug classes.  Shapes: the smallest legal plan; ragged stem tiles and one partial conv2
tile; odd conv map (live -inf pool padding); exactly one full conv2 tile and three LSTM passes; a 1-wide ragged stem edge, three
conv2 tiles with a tail, hidden = 130 and a capacity above the clip count.  And conv2 bit for bit as what it is built from: the
fp32 convolution primitive on the pooled tap, summed on the host in the order of csrc/rva_mfma_f32.h's tile sum.

Observed / bound: every test prints it per stage (``pytest -s``).  On the CPU torch's fp32 operators sit at 0.00 .. 0.58 of
the bounds (the mean is the tightest)."""
import ctypes as C

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.clip_plan import FusedCnnLstm
from tests import clip_stage_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
STAGES = ("pooled", "partial", "feat", "gx", "h1", "h2")
GEOMETRY = {R.LSTM_SHAPES[0]: ((1, 1), 1), R.LSTM_SHAPES[1]: ((10, 14), 1), R.LSTM_SHAPES[2]: ((8, 9), 1),
            R.LSTM_SHAPES[3]: ((16, 16), 1), R.LSTM_SHAPES[4]: ((17, 33), 3)}        # pooled map, conv2 tiles


def _run(plan, ring, index, n):
    logits = plan.run(ring, index, n).clone()
    taps = {k: plan.stage(k, n) for k in STAGES}
    taps["logits"] = logits
    return taps


@pytest.mark.parametrize("shape", R.LSTM_SHAPES, ids=R.shape_id)
def test_every_stage_against_float64(shape):
    """The LSTM bound is 64 x e_ref (torch's fp32 LSTM against float64 on the same features), floored at 1e-6."""
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips = R.lstm_case(shape)
    plan = FusedCnnLstm(net, (H, W), T, cap)
    assert (plan.pooled_hw, plan.conv2_tiles) == GEOMETRY[shape]
    ring = clips.to(DEV).view(-1, 3, H, W).contiguous()
    taps = _run(plan, ring, torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    assert tuple(taps["h1"].shape) == (T, n, hidden) and tuple(taps["gx"].shape) == (n, T, 4 * hidden)
    refs = R.lstm_refs({k: v.cpu() for k, v in taps.items()}, clips, p, shape)
    e_ref, bound = refs["_lstm"]
    print(f"{R.shape_id(shape)}: e_ref {e_ref:.3e}, LSTM bound {bound:.3e}")
    bad = []
    for k in STAGES + ("logits",):
        R.report(shape, k, taps[k].cpu(), *refs[k], out=bad)
    assert not bad, bad


def test_stages_through_a_permuted_index_table_are_bit_equal():
    shape = R.LSTM_SHAPES[4]
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips = R.lstm_case(shape)
    plan = FusedCnnLstm(net, (H, W), T, cap)
    frames = clips.to(DEV).view(-1, 3, H, W).contiguous()
    want = _run(plan, frames, torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    slots = n * T + 5                                       # a ring larger than the clips, frames scattered over it
    perm = torch.randperm(slots, generator=torch.Generator().manual_seed(9))[:n * T]
    ring = torch.full((slots, 3, H, W), float("nan"), device=DEV)
    ring[perm] = frames
    got = _run(plan, ring, perm.to(torch.int32).to(DEV), n)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_conv2_is_the_f32_conv_primitive_summed_in_the_documented_order():
    """k_clip_conv2 and rva_conv2d_nhwc_f32_v share one MFMA core (csrc/rva_mfma_f32.h): on the pooled tap the primitive (Cin 64,
    Cout 128, k 3, stride 1, no activation, the plan's bias; variant 0 and every forced variant) gives conv2's map before the
    ReLU, and that map summed in fp32 on the host in the tile sum's documented order is the ``partial`` tap, bit for bit.
    17 x 33 = 561 pixels: three tiles, the last one ragged."""
    shape = R.LSTM_SHAPES[4]
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips = R.lstm_case(shape)
    plan = FusedCnnLstm(net, (H, W), T, cap)
    taps = _run(plan, clips.to(DEV).view(-1, 3, H, W).contiguous(), torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    pooled, partial = taps["pooled"], taps["partial"].cpu().numpy()
    F_, Hp, Wp = pooled.shape[:3]
    assert (F_, Hp, Wp, partial.shape) == (n * T, 17, 33, (n * T, 3, 128))
    w = p["conv2_w"].permute(0, 2, 3, 1).contiguous().float().to(DEV)          # [co][ci][ky][kx] -> [co][tap][ci]
    b = p["conv2_b"].float().to(DEV)
    variants = range(int(plan.L.rva_conv_f32_num_variants()) + 1)
    assert len(variants) >= 2
    for v in variants:
        out = torch.full((F_, Hp, Wp, 128), float("nan"), device=DEV)
        plan.ctx.check(plan.L.rva_conv2d_nhwc_f32_v(plan.ctx.handle, C.c_void_p(pooled.data_ptr()), 64, C.c_void_p(w.data_ptr()),
                                                    C.c_void_p(b.data_ptr()), C.c_void_p(out.data_ptr()), 128, None, 0, F_, Hp, Wp,
                                                    64, 128, 3, 1, 0, v, ops._stream_ptr()),
                       "rva_conv2d_nhwc_f32_v")
        got = R.tile_partial_in_kernel_order(out.cpu().numpy().reshape(F_, Hp * Wp, 128))
        assert got.dtype == np.float32 and np.array_equal(got, partial), ("variant", v)


def test_tap_contract():
    shape = R.LSTM_SHAPES[1]
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips = R.lstm_case(shape)
    plan = FusedCnnLstm(net, (H, W), T, cap)
    fn, st = plan.L.rva_cnnlstm_plan_stage, ops._stream_ptr()
    count = C.c_int64(-1)
    want = {0: n * T * 10 * 14 * 64, 1: n * T * 128, 2: n * T * 128, 3: n * T * 4 * hidden, 4: n * T * hidden, 5: n * T * hidden}
    for stage, floats in want.items():                      # dst == NULL reports the count (before any run, too)
        assert fn(plan.handle, stage, n, None, 0, C.byref(count), st) == N.RVA_OK and count.value == floats
    assert fn(plan.handle, 2, 1, None, 0, C.byref(count), st) == N.RVA_OK and count.value == T * 128
    plan.run(clips.to(DEV).view(-1, 3, H, W).contiguous(), torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    dst = torch.full((want[2] + 8,), -7.0, device=DEV)
    ptr = C.c_void_p(dst.data_ptr())
    for bad in ((6, n, ptr, dst.numel()), (-1, n, ptr, dst.numel()), (2, n, ptr, want[2] - 1), (2, cap + 1, ptr, 1 << 30),
                (2, 0, ptr, dst.numel())):
        assert fn(plan.handle, *bad, None, st) == N.RVA_ERR_ARG, bad
    assert fn(None, 2, n, ptr, dst.numel(), None, st) == N.RVA_ERR_ARG
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())                        # a refused call copies nothing
    assert fn(plan.handle, 2, n, ptr, dst.numel(), C.byref(count), st) == N.RVA_OK and count.value == want[2]
    assert torch.equal(dst[:want[2]].view(n * T, 128), plan.stage("feat", n)) and bool((dst[want[2]:] == -7.0).all())
    with pytest.raises(ValueError, match="unknown stage"):
        plan.stage("conv2", n)
    with pytest.raises(RuntimeError, match="capacity"):
        plan.stage("feat", cap + 1)
