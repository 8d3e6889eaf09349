"""Every stage of the fp32 ResNet-18 plan (csrc/rva_resnet.hip) against float64 on the GPU, through the read-only workspace tap
``rva_resnet_plan_stage``: the stem's pooled map, each block's first convolution, the three shortcut convolutions, each block's
output, the mean and the logits.  Each stage's reference is computed from the tap(s) the kernel itself read, with the derived
bounds of tests/resnet_stage_refs.py, so a failure names the launch; tests/test_resnet_stages_host.py proves on the CPU that
these bounds see k_res_conv's bug classes.  The sharpest check is bit-equality: k_res_conv and rva_conv2d_nhwc_f32_v share one
MFMA core and one reduction order (csrc/rva_mfma_f32.h), so every block convolution must equal the primitive on the same tap.

Shapes: a one-pixel layer4 (eight of nine taps are padding); odd maps whose row counts are never a multiple of 32, tiles that
span images and a capacity above the batch; non-square maps with 37 classes; several row tiles per layer, each with a tail.

Observed / bound: every test prints it per stage (``pytest -s``).  On the CPU torch's fp32 operators sit at <= 0.06 of the
convolutions' bounds and <= 0.47 of the mean's."""
import ctypes as C

import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.clip_plan import FusedCnnLstm
from realtime_video_analytics_32streams_amd.resnet_plan import FusedResNet18, resnet_maps
from realtime_video_analytics_32streams_amd.temporal import CnnLstmNet
from tests import resnet_stage_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _run(plan, frames, index, n):
    logits = plan.run(frames, index, n).clone()
    taps = {k: plan.stage(k, n) for k in R.STAGES}
    taps["logits"] = logits
    return taps


def _plan(shape):
    B, H, W, classes, cap = shape
    net, p, frames = R.case(shape)
    plan = FusedResNet18(net, (H, W), cap)
    assert plan.maps == resnet_maps(H, W) and plan.n_launches == 22
    return net, p, frames, plan


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_every_stage_against_float64_and_the_conv_primitive(shape):
    B, H, W, classes, cap = shape
    net, p, frames, plan = _plan(shape)
    taps = _run(plan, frames.to(DEV).contiguous(), torch.arange(B, dtype=torch.int32, device=DEV), B)
    refs = R.refs({k: v.cpu() for k, v in taps.items()}, frames, p, shape)
    bad = []
    for k in R.STAGES + ("logits",):
        R.report(shape, k, taps[k].cpu(), *refs[k], out=bad)
    assert not bad, bad
    # bit-equality with rva_conv2d_nhwc_f32_v (variant 0, no activation) on the tap the launch read
    packed = {k: torch.from_numpy(v).to(DEV) for k, v in R.pack_resnet18(net).items()}

    def prim(name, x, res=None):
        i = R.CONV_OF[name]
        cin, c, s = R.BLOCKS[int(name[-1])]
        k, stride, ci = (1, 2, cin) if name.startswith("down") else (3, s, cin) if name.startswith("mid") else (3, 1, c)
        out = torch.full_like(taps[name], float("nan"))
        plan.ctx.check(plan.L.rva_conv2d_nhwc_f32_v(
            plan.ctx.handle, C.c_void_p(x.data_ptr()), ci, C.c_void_p(packed[f"c{i}_w"].data_ptr()), C.c_void_p(packed[f"c{i}_b"].data_ptr()),
            C.c_void_p(out.data_ptr()), c, C.c_void_p(res.data_ptr()) if res is not None else None, c if res is not None else 0,
            B, x.shape[1], x.shape[2], ci, c, k, stride, 0, 0, ops._stream_ptr()), "rva_conv2d_nhwc_f32_v")
        return out

    prev = "pooled"
    for b in range(8):
        x = taps[prev]
        assert torch.equal(taps[f"mid{b}"], torch.relu(prim(f"mid{b}", x))), f"mid{b}"
        r = x
        if b in R.DOWN:
            assert torch.equal(taps[f"down{b}"], prim(f"down{b}", x)), f"down{b}"
            r = taps[f"down{b}"]
        assert torch.equal(taps[f"out{b}"], torch.relu(prim(f"out{b}", taps[f"mid{b}"], r))), f"out{b}"
        prev = f"out{b}"


def test_pooled_is_the_cnnlstm_plans_pooled_tap():
    """One stem kernel serves both plans (rva_clip_stem_launch): the same frames and stem weights give the same bits."""
    shape = R.SHAPES[2]
    B, H, W, classes, cap = shape
    net, p, frames, plan = _plan(shape)
    lstm = R.synth.seeded_module(lambda: CnnLstmNet(5, 16), 11)
    with torch.no_grad():                                    # the ResNet's stem (no conv bias) in the CNN-LSTM's stem
        lstm.stem[0].weight.copy_(net.stem[0].weight)
        lstm.stem[0].bias.zero_()
        for a in ("weight", "bias", "running_mean", "running_var"):
            getattr(lstm.stem[1], a).copy_(getattr(net.stem[1], a))
    other = FusedCnnLstm(lstm, (H, W), 1, B)
    x = frames.to(DEV).contiguous()
    iota = torch.arange(B, dtype=torch.int32, device=DEV)
    plan.run(x, iota, B)
    other.run(x, iota, B)
    assert torch.equal(plan.stage("pooled", B), other.stage("pooled", B))


def test_stages_through_a_permuted_index_table_are_bit_equal():
    shape = R.SHAPES[2]
    B, H, W, classes, cap = shape
    net, p, frames, plan = _plan(shape)
    flat = frames.to(DEV).contiguous()
    want = _run(plan, flat, torch.arange(B, dtype=torch.int32, device=DEV), B)
    slots = B + 5
    perm = torch.randperm(slots, generator=torch.Generator().manual_seed(9))[:B]
    ring = torch.full((slots, 3, H, W), float("nan"), device=DEV)
    ring[perm] = flat
    got = _run(plan, ring, perm.to(torch.int32).to(DEV), B)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_tap_contract():
    shape = R.SHAPES[1]
    B, H, W, classes, cap = shape                            # maps 9 -> 5 -> 3 -> 2, capacity 4 above the batch of 3
    net, p, frames, plan = _plan(shape)
    fn, st = plan.L.rva_resnet_plan_stage, ops._stream_ptr()
    count = C.c_int64(-1)
    want = {0: B * 81 * 64, 1: B * 81 * 64, 8: B * 4 * 512, 9: B * 25 * 128, 10: B * 9 * 256, 11: B * 4 * 512, 12: B * 81 * 64, 14: B * 25 * 128,
            19: B * 4 * 512, 20: B * 512}
    for stage, floats in want.items():                      # dst == NULL reports the count (before any run, too)
        assert fn(plan.handle, stage, B, None, 0, C.byref(count), st) == N.RVA_OK and count.value == floats, stage
    assert fn(plan.handle, 20, cap, None, 0, C.byref(count), st) == N.RVA_OK and count.value == cap * 512
    plan.run(frames.to(DEV).contiguous(), torch.arange(B, dtype=torch.int32, device=DEV), B)
    dst = torch.full((want[20] + 8,), -7.0, device=DEV)
    ptr = C.c_void_p(dst.data_ptr())
    for bad in ((21, B, ptr, dst.numel()), (-1, B, ptr, dst.numel()), (20, B, ptr, want[20] - 1), (20, cap + 1, ptr, 1 << 30),
                (20, 0, ptr, dst.numel())):
        assert fn(plan.handle, *bad, None, st) == N.RVA_ERR_ARG, bad
    assert fn(None, 20, B, ptr, dst.numel(), None, st) == N.RVA_ERR_ARG
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())                        # a refused call copies nothing
    assert fn(plan.handle, 20, B, ptr, dst.numel(), C.byref(count), st) == N.RVA_OK and count.value == want[20]
    assert torch.equal(dst[:want[20]].view(B, 512), plan.stage("feat", B)) and bool((dst[want[20]:] == -7.0).all())
    with pytest.raises(ValueError, match="unknown stage"):
        plan.stage("down3", B)
    with pytest.raises(RuntimeError, match="capacity"):
        plan.stage("feat", cap + 1)
