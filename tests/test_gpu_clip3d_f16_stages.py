"""Every stage of the fp16 3D-CNN clip plan (csrc/rva_clip3d.hip) against float64 on the GPU, through the read-only workspace
tap ``rva_cnn3d_f16_plan_stage``: conv1's pooled fp16 map (fp16 frames with an odd row length, zero temporal padding), conv2's
pooled fp16 map (the fp16 MFMA's lane-half operand layout, the pool-in-epilogue shuffle), conv3's fp32 tile partials, the mean
and the logits.  Each stage's reference is computed from the tap of the stage before it with the bounds of
tests/clip3d_f16_refs.py, so a failure names the kernel; tests/test_clip3d_f16_host.py proves on the CPU that these bounds see
the kernels' bug classes.  Shapes: those of tests/test_gpu_clip3d_stages.py.  Every test prints observed / bound per stage
(``pytest -s``); on an MI355X: act1 0.90 .. 0.97 (the fp16 rounding itself), act2 0.32 .. 0.43, partial 0.00, feat 0.00 .. 0.56,
logits 0.00."""
import ctypes as C

import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.clip_plan import Fused3dCnnF16
from tests import clip3d_f16_refs as Q
from tests import clip_stage_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
GEOMETRY = {R.C3D_SHAPES[0]: ((2, 2, 2), (1, 1, 1), (1, 1, 1)), R.C3D_SHAPES[1]: ((7, 12, 20), (3, 6, 10), (6, 6, 1)),
            R.C3D_SHAPES[2]: ((4, 18, 34), (2, 9, 17), (15, 10, 2))}                  # pool1, pool2, tiles of conv1 / conv2 / conv3


def _run(plan, ring, index, n):
    logits = plan.run(ring, index, n).clone()
    taps = {k: plan.stage(k, n) for k in Q.STAGES}
    taps["logits"] = logits
    return taps


@pytest.mark.parametrize("shape", R.C3D_SHAPES, ids=R.shape_id)
def test_every_stage_against_float64(shape):
    T, H, W, classes, n, cap = shape
    net, p, frames16 = Q.c3d16_case(shape)
    plan = Fused3dCnnF16(net, (H, W), T, cap)
    assert (plan.pool1, plan.pool2, plan.tiles, plan.n_launches) == (*GEOMETRY[shape], 5)
    ring = frames16.to(DEV).view(-1, 3, H, W).contiguous()
    taps = _run(plan, ring, torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    assert taps["act1"].dtype == taps["act2"].dtype == torch.float16
    assert taps["partial"].dtype == taps["feat"].dtype == taps["logits"].dtype == torch.float32
    refs = Q.c3d16_refs({k: v.cpu() for k, v in taps.items()}, frames16, p, shape)
    bad = []
    for k in Q.STAGES + ("logits",):
        R.report(shape, k, taps[k].cpu(), *refs[k], out=bad)
    assert not bad, bad


def test_stages_through_a_permuted_index_table_over_a_nan_ring_are_bit_equal():
    shape = R.C3D_SHAPES[2]
    T, H, W, classes, n, cap = shape
    net, p, frames16 = Q.c3d16_case(shape)
    plan = Fused3dCnnF16(net, (H, W), T, cap)
    flat = frames16.to(DEV).view(-1, 3, H, W).contiguous()
    want = _run(plan, flat, torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    slots = n * T + 5
    perm = torch.randperm(slots, generator=torch.Generator().manual_seed(9))[:n * T]
    ring = torch.full((slots, 3, H, W), float("nan"), dtype=torch.float16, device=DEV)
    ring[perm] = flat
    got = _run(plan, ring, perm.to(torch.int32).to(DEV), n)
    for k in want:
        assert not bool(torch.isnan(got[k].float()).any()), k
        assert torch.equal(got[k], want[k]), k


def test_tap_contract():
    shape = R.C3D_SHAPES[2]
    T, H, W, classes, n, cap = shape
    net, p, frames16 = Q.c3d16_case(shape)
    plan = Fused3dCnnF16(net, (H, W), T, cap)
    fn, st = plan.L.rva_cnn3d_f16_plan_stage, ops._stream_ptr()
    count = C.c_int64(-1)
    want = {0: n * T * 18 * 34 * 64, 1: n * 306 * 128, 2: n * 2 * 256, 3: n * 256}            # ELEMENT counts
    for stage, elems in want.items():                       # dst == NULL reports the count (before any run, too)
        assert fn(plan.handle, stage, n, None, 0, C.byref(count), st) == N.RVA_OK and count.value == elems
    assert fn(plan.handle, 3, cap, None, 0, C.byref(count), st) == N.RVA_OK and count.value == cap * 256
    ring = frames16.to(DEV).view(-1, 3, H, W).contiguous()
    with pytest.raises(ValueError, match="fp16"):
        plan.run(ring.float(), torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    plan.run(ring, torch.arange(n * T, dtype=torch.int32, device=DEV), n)
    dst = torch.full((want[3] + 8,), -7.0, device=DEV)
    ptr = C.c_void_p(dst.data_ptr())
    for bad in ((4, n, ptr, dst.numel()), (-1, n, ptr, dst.numel()), (3, n, ptr, want[3] - 1), (3, cap + 1, ptr, 1 << 30),
                (3, 0, ptr, dst.numel())):
        assert fn(plan.handle, *bad, None, st) == N.RVA_ERR_ARG, bad
    assert fn(None, 3, n, ptr, dst.numel(), None, st) == N.RVA_ERR_ARG
    # an fp16 stage counts fp16 elements: room for one element less is refused, and exactly `count` halves are written
    h = torch.full((want[1] + 8,), -7.0, dtype=torch.float16, device=DEV)
    hp = C.c_void_p(h.data_ptr())
    assert fn(plan.handle, 1, n, hp, want[1] - 1, None, st) == N.RVA_ERR_ARG
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all()) and bool((h == -7.0).all())                       # a refused call copies nothing
    assert fn(plan.handle, 3, n, ptr, dst.numel(), C.byref(count), st) == N.RVA_OK and count.value == want[3]
    assert torch.equal(dst[:want[3]].view(n, 256), plan.stage("feat", n)) and bool((dst[want[3]:] == -7.0).all())
    assert fn(plan.handle, 1, n, hp, want[1], C.byref(count), st) == N.RVA_OK and count.value == want[1]
    assert torch.equal(h[:want[1]].view(n, 306, 128), plan.stage("act2", n)) and bool((h[want[1]:] == -7.0).all())
    assert plan.stage("act1", n).shape == (n, T, 18, 34, 64) and plan.stage("act1", n).dtype == torch.float16
    with pytest.raises(ValueError, match="unknown stage"):
        plan.stage("conv3", n)
    with pytest.raises(RuntimeError, match="capacity"):
        plan.stage("feat", cap + 1)
