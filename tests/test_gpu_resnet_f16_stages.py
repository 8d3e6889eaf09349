"""Every stage of the fp16 ResNet-18 plan (csrc/rva_resnet_f16.hip, engine ``resnet-f16``) against float64 on the GPU, through the
workspace tap ``rva_resnet_f16_plan_stage``: the MFMA stem's fp16 ``pooled``, each block's first convolution, the three shortcut
convolutions, each block's output, the mean and the logits.  Each reference is computed from the tap(s) the kernel itself read,
on the fp16-rounded weights the plan holds, with the bounds of tests/resnet_f16_refs.py, so a failure names the launch;
tests/test_resnet_f16_host.py proves on the CPU that these bounds see k_res16_conv's bug classes.

Shapes: ``resnet_stage_refs.SHAPES`` as they are (a one-pixel layer4; odd maps 17 / 9 / 5 / 3 / 2 with live pool padding and a
capacity above the batch; non-square maps with a class tail; 17 frames: tiles that span images, row tails).  Every tile of the
kernel's table must leave the same bits (``RVA_RES16_TILE`` forces one at plan creation), ``pooled`` must be the CNN-LSTM fp16
plan's ``pooled`` (one stem kernel serves both), and a permuted index table into a larger NaN-filled ring changes no bit.

Observed / bound: every test prints it per stage (``pytest -s``)."""
import ctypes as C

import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.clip_plan import FusedCnnLstmF16
from realtime_video_analytics_32streams_amd.resnet_plan import FusedResNet18F16, resnet_maps
from realtime_video_analytics_32streams_amd.temporal import CnnLstmNet
from tests import resnet_f16_refs as Q
from tests import resnet_stage_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _run(plan, frames, index, n):
    logits = plan.run(frames, index, n).clone()
    taps = {k: plan.stage(k, n) for k in Q.STAGES}
    taps["logits"] = logits
    return taps


def _plan(shape):
    B, H, W, classes, cap = shape
    net, p, frames16 = Q.case16(shape)
    plan = FusedResNet18F16(net, (H, W), cap)
    assert plan.maps == resnet_maps(H, W) and plan.n_launches == 22
    return net, p, frames16, plan


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_every_stage_against_float64(shape):
    B, H, W, classes, cap = shape
    net, p, frames16, plan = _plan(shape)
    taps = _run(plan, frames16.to(DEV).contiguous(), torch.arange(B, dtype=torch.int32, device=DEV), B)
    for k in Q.STAGES + ("logits",):
        assert taps[k].dtype == (torch.float16 if k in Q.F16_STAGES else torch.float32), k
    assert tuple(taps["out7"].shape) == (B, *plan.maps[4], 512) and tuple(taps["logits"].shape) == (B, classes)
    refs = Q.refs16({k: v.cpu() for k, v in taps.items()}, frames16, p, shape)
    bad = []
    for k in Q.STAGES + ("logits",):
        R.report(shape, k, taps[k].cpu(), *refs[k], out=bad)
    assert not bad, bad
    assert all(bool((taps[k] != 0).any()) for k in Q.STAGES)


@pytest.mark.parametrize("shape", [R.SHAPES[1], R.SHAPES[3]], ids=R.shape_id)
def test_every_tile_of_the_table_leaves_the_same_bits(shape, monkeypatch):
    B, H, W, classes, cap = shape
    net, p, frames16, plan = _plan(shape)
    x, iota = frames16.to(DEV).contiguous(), torch.arange(B, dtype=torch.int32, device=DEV)
    want = _run(plan, x, iota, B)
    for tile in range(5):
        monkeypatch.setenv("RVA_RES16_TILE", str(tile))               # read at plan creation
        got = _run(FusedResNet18F16(net, (H, W), cap), x, iota, B)
        for k in want:
            assert torch.equal(got[k], want[k]), (tile, k)


def test_pooled_is_the_cnnlstm_f16_plans_pooled_tap():
    """One stem kernel serves both plans (rva_clip16_stem_launch): the same frames and stem weights give the same bits."""
    shape = R.SHAPES[2]
    B, H, W, classes, cap = shape
    net, p, frames16, plan = _plan(shape)
    lstm = R.synth.seeded_module(lambda: CnnLstmNet(5, 16), 11)
    with torch.no_grad():                                    # the ResNet's stem (no conv bias) in the CNN-LSTM's stem
        lstm.stem[0].weight.copy_(net.stem[0].weight)
        lstm.stem[0].bias.zero_()
        for a in ("weight", "bias", "running_mean", "running_var"):
            getattr(lstm.stem[1], a).copy_(getattr(net.stem[1], a))
    other = FusedCnnLstmF16(lstm, (H, W), 1, B)
    x = frames16.to(DEV).contiguous()
    iota = torch.arange(B, dtype=torch.int32, device=DEV)
    plan.run(x, iota, B)
    other.run(x, iota, B)
    a, b = plan.stage("pooled", B), other.stage("pooled", B)
    assert a.dtype == b.dtype == torch.float16 and torch.equal(a, b) and bool((a != 0).any())


def test_stages_through_a_permuted_index_table_are_bit_equal():
    shape = R.SHAPES[2]
    B, H, W, classes, cap = shape
    net, p, frames16, plan = _plan(shape)
    flat = frames16.to(DEV).contiguous()
    want = _run(plan, flat, torch.arange(B, dtype=torch.int32, device=DEV), B)
    slots = B + 5
    perm = torch.randperm(slots, generator=torch.Generator().manual_seed(9))[:B]
    ring = torch.full((slots, 3, H, W), float("nan"), dtype=torch.float16, device=DEV)
    ring[perm] = flat
    got = _run(plan, ring, perm.to(torch.int32).to(DEV), B)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_tap_contract_counts_elements_of_the_stored_type():
    shape = R.SHAPES[1]
    B, H, W, classes, cap = shape                            # maps 9 -> 5 -> 3 -> 2, capacity 4 above the batch of 3
    net, p, frames16, plan = _plan(shape)
    fn, st = plan.L.rva_resnet_f16_plan_stage, ops._stream_ptr()
    count = C.c_int64(-1)
    want = {0: B * 81 * 64, 1: B * 81 * 64, 8: B * 4 * 512, 9: B * 25 * 128, 10: B * 9 * 256, 11: B * 4 * 512, 12: B * 81 * 64, 14: B * 25 * 128,
            19: B * 4 * 512, 20: B * 512}
    for stage, elems in want.items():                       # dst == NULL reports the count (before any run, too)
        assert fn(plan.handle, stage, B, None, 0, C.byref(count), st) == N.RVA_OK and count.value == elems, stage
    assert fn(plan.handle, 20, cap, None, 0, C.byref(count), st) == N.RVA_OK and count.value == cap * 512
    plan.run(frames16.to(DEV).contiguous(), torch.arange(B, dtype=torch.int32, device=DEV), B)
    for stage, dtype, name in ((18, torch.float16, "out6"), (19, torch.float32, "out7"), (20, torch.float32, "feat")):
        dst = torch.full((want.get(stage, B * 4 * 512) + 8,), -7.0, dtype=dtype, device=DEV)
        n_el = dst.numel() - 8
        ptr = C.c_void_p(dst.data_ptr())
        for bad in ((21, B, ptr, dst.numel()), (-1, B, ptr, dst.numel()), (stage, B, ptr, n_el - 1), (stage, cap + 1, ptr, 1 << 30),
                    (stage, 0, ptr, dst.numel())):
            assert fn(plan.handle, *bad, None, st) == N.RVA_ERR_ARG, bad
        assert fn(None, stage, B, ptr, dst.numel(), None, st) == N.RVA_ERR_ARG
        torch.cuda.synchronize()
        assert bool((dst == -7.0).all())                    # a refused call copies nothing
        assert fn(plan.handle, stage, B, ptr, dst.numel(), C.byref(count), st) == N.RVA_OK and count.value == n_el
        got = plan.stage(name, B)
        assert got.dtype == dtype and torch.equal(dst[:n_el].view(got.shape), got) and bool((dst[n_el:] == -7.0).all())
    with pytest.raises(ValueError, match="unknown stage"):
        plan.stage("down3", B)
    with pytest.raises(RuntimeError, match="capacity"):
        plan.stage("feat", cap + 1)
