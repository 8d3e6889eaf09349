"""Every stage of the fp32 3D-CNN clip plan (csrc/rva_clip3d.hip) against float64 on the GPU, through the read-only workspace
tap ``rva_cnn3d_plan_stage``: conv1's pooled map (zero temporal padding at both ends, dropped odd row, column and frame),
conv2's pooled map (the pool-in-epilogue lane shuffle), conv3's tile partials, the mean and the logits.  Each stage's
reference is computed from the tap of the stage before it with the bounds of tests/clip_stage_refs.py, so a failure names the
kernel; tests/test_clip_stages_host.py proves on the CPU that these bounds see the kernels' bug classes.  Shapes: one pool
group; the odd shape (conv2 tail of 20 groups, one partial conv3 tile); ragged conv1 tiles, 10 conv2 tiles with a tail of 18, 2
conv3 tiles with a tail of 50 and a capacity above the clip count.

Observed / bound: every test prints it per stage (``pytest -s``).  These tests have not run on a GPU yet; on the
CPU torch's fp32 operators sit at 0.00 .. 0.58 of the bounds (the mean is the tightest)."""
import ctypes as C

import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.clip_plan import Fused3dCnn
from tests import clip_stage_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
STAGES = ("act1", "act2", "partial", "feat")
GEOMETRY = {R.C3D_SHAPES[0]: ((2, 2, 2), (1, 1, 1), (1, 1, 1)), R.C3D_SHAPES[1]: ((7, 12, 20), (3, 6, 10), (6, 6, 1)),
            R.C3D_SHAPES[2]: ((4, 18, 34), (2, 9, 17), (15, 10, 2))}                  # pool1, pool2, tiles of conv1 / conv2 / conv3


def _run(plan, ring, index, n):
    logits = plan.run(ring, index, n).clone()
    taps = {k: plan.stage(k, n) for k in STAGES}
    taps["logits"] = logits
    return taps


@pytest.mark.parametrize("shape", R.C3D_SHAPES, ids=R.shape_id)
def test_every_stage_against_float64(shape):
    T, H, W, classes, n, cap = shape
    net, p, frames = R.c3d_case(shape)
    plan = Fused3dCnn(net, (H, W), T, cap)
    assert (plan.pool1, plan.pool2, plan.tiles) == GEOMETRY[shape]
    ring = frames.to(DEV).view(-1, 3, H, W).contiguous()
    taps = _run(plan, ring, torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    refs = R.c3d_refs({k: v.cpu() for k, v in taps.items()}, frames, p, shape)
    bad = []
    for k in STAGES + ("logits",):
        R.report(shape, k, taps[k].cpu(), *refs[k], out=bad)
    assert not bad, bad


def test_stages_through_a_permuted_index_table_are_bit_equal():
    shape = R.C3D_SHAPES[2]
    T, H, W, classes, n, cap = shape
    net, p, frames = R.c3d_case(shape)
    plan = Fused3dCnn(net, (H, W), T, cap)
    flat = frames.to(DEV).view(-1, 3, H, W).contiguous()
    want = _run(plan, flat, torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    slots = n * T + 5
    perm = torch.randperm(slots, generator=torch.Generator().manual_seed(9))[:n * T]
    ring = torch.full((slots, 3, H, W), float("nan"), device=DEV)
    ring[perm] = flat
    got = _run(plan, ring, perm.to(torch.int32).to(DEV), n)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_tap_contract():
    shape = R.C3D_SHAPES[2]
    T, H, W, classes, n, cap = shape
    net, p, frames = R.c3d_case(shape)
    plan = Fused3dCnn(net, (H, W), T, cap)
    fn, st = plan.L.rva_cnn3d_plan_stage, ops._stream_ptr()
    count = C.c_int64(-1)
    want = {0: n * T * 18 * 34 * 64, 1: n * 306 * 128, 2: n * 2 * 256, 3: n * 256}
    for stage, floats in want.items():                      # dst == NULL reports the count (before any run, too)
        assert fn(plan.handle, stage, n, None, 0, C.byref(count), st) == N.RVA_OK and count.value == floats
    assert fn(plan.handle, 3, cap, None, 0, C.byref(count), st) == N.RVA_OK and count.value == cap * 256
    plan.run(frames.to(DEV).view(-1, 3, H, W).contiguous(), torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    dst = torch.full((want[3] + 8,), -7.0, device=DEV)
    ptr = C.c_void_p(dst.data_ptr())
    for bad in ((4, n, ptr, dst.numel()), (-1, n, ptr, dst.numel()), (3, n, ptr, want[3] - 1), (3, cap + 1, ptr, 1 << 30),
                (3, 0, ptr, dst.numel())):
        assert fn(plan.handle, *bad, None, st) == N.RVA_ERR_ARG, bad
    assert fn(None, 3, n, ptr, dst.numel(), None, st) == N.RVA_ERR_ARG
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())                        # a refused call copies nothing
    assert fn(plan.handle, 3, n, ptr, dst.numel(), C.byref(count), st) == N.RVA_OK and count.value == want[3]
    assert torch.equal(dst[:want[3]].view(n, 256), plan.stage("feat", n)) and bool((dst[want[3]:] == -7.0).all())
    with pytest.raises(ValueError, match="unknown stage"):
        plan.stage("conv3", n)
    with pytest.raises(RuntimeError, match="capacity"):
        plan.stage("feat", cap + 1)
