"""Every stage of the fp16 CNN-LSTM clip plan (csrc/rva_clip_f16.hip, engine ``clip-f16``) against float64 on the GPU, through
the workspace tap ``rva_cnnlstm_f16_plan_stage``: the MFMA stem's fp16 ``pooled``, conv2's tile partials, the spatial mean, layer
1's input projection, both LSTM layers at every step and clip, and the logits.  Each reference is computed from the tap of the
stage before it with the bounds of tests/clip_f16_refs.py, so a failure names the kernel; tests/test_clip_f16_host.py proves on the
CPU that these bounds see the kernels' bug classes.  Shapes: ``clip_stage_refs.LSTM_SHAPES`` as they are (single pixel; ragged stem
tiles; odd conv map with live -inf pool padding; 17 clips = three LSTM passes; odd width, three conv2 tiles with a tail, hidden =
130 -- a ragged k-slice -- and a capacity above the clip count).  And conv2's two forms (weights through LDS or not) bit for bit.

Observed / bound: every test prints it per stage (``pytest -s``)."""
import ctypes as C

import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.clip_plan import FusedCnnLstmF16
from tests import clip_f16_refs as Q
from tests import clip_stage_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
GEOMETRY = {R.LSTM_SHAPES[0]: ((1, 1), 1), R.LSTM_SHAPES[1]: ((10, 14), 1), R.LSTM_SHAPES[2]: ((8, 9), 1),
            R.LSTM_SHAPES[3]: ((16, 16), 1), R.LSTM_SHAPES[4]: ((17, 33), 3)}        # pooled map, conv2 tiles


def _run(plan, ring, index, n):
    logits = plan.run(ring, index, n).clone()
    taps = {k: plan.stage(k, n) for k in Q.STAGES}
    taps["logits"] = logits
    return taps


def _case(shape):
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips16 = Q.lstm16_case(shape)
    ring = clips16.to(DEV).view(-1, 3, H, W).contiguous()
    return net, p, clips16, ring, torch.arange(n * T, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("shape", R.LSTM_SHAPES, ids=R.shape_id)
def test_every_stage_against_float64(shape):
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips16, ring, iota = _case(shape)
    plan = FusedCnnLstmF16(net, (H, W), T, cap)
    assert (plan.pooled_hw, plan.conv2_tiles) == GEOMETRY[shape] and plan.n_launches == 4 + T + 1 + 1
    taps = _run(plan, ring, iota, n)
    assert taps["pooled"].dtype == torch.float16 and all(taps[k].dtype == torch.float32 for k in Q.STAGES[1:] + ("logits",))
    assert tuple(taps["h1"].shape) == (T, n, hidden) and tuple(taps["gx"].shape) == (n, T, 4 * hidden)
    refs = Q.lstm16_refs({k: v.cpu() for k, v in taps.items()}, clips16, p, shape)
    e_ref, bound = refs["_lstm"]
    print(f"{R.shape_id(shape)}: e_ref {e_ref:.3e}, LSTM bound {bound:.3e}")
    bad = []
    for k in Q.STAGES + ("logits",):
        R.report(shape, k, taps[k].cpu(), *refs[k], out=bad)
    assert not bad, bad


@pytest.mark.parametrize("shape", [R.LSTM_SHAPES[1], R.LSTM_SHAPES[4]], ids=R.shape_id)
def test_conv2_with_and_without_the_lds_weight_stage_is_bit_identical(shape, monkeypatch):
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips16, ring, iota = _case(shape)
    taps = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RVA_CLIP16_WLDS", mode)               # read at plan creation
        taps[mode] = _run(FusedCnnLstmF16(net, (H, W), T, cap), ring, iota, n)
    for k in taps["1"]:
        assert torch.equal(taps["1"][k], taps["0"][k]), k
    assert bool((taps["1"]["partial"] != 0).any())


def test_stages_through_a_permuted_index_table_are_bit_equal():
    shape = R.LSTM_SHAPES[4]
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips16, frames, iota = _case(shape)
    plan = FusedCnnLstmF16(net, (H, W), T, cap)
    want = _run(plan, frames, iota, n)
    slots = n * T + 5                                       # a ring larger than the clips, frames scattered over it
    perm = torch.randperm(slots, generator=torch.Generator().manual_seed(9))[:n * T]
    ring = torch.full((slots, 3, H, W), float("nan"), dtype=torch.float16, device=DEV)
    ring[perm] = frames
    got = _run(plan, ring, perm.to(torch.int32).to(DEV), n)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_tap_contract_counts_elements_and_delivers_pooled_as_fp16():
    shape = R.LSTM_SHAPES[1]
    H, W, T, hidden, classes, n, cap = shape
    net, p, clips16, ring, iota = _case(shape)
    plan = FusedCnnLstmF16(net, (H, W), T, cap)
    fn, st = plan.L.rva_cnnlstm_f16_plan_stage, ops._stream_ptr()
    count = C.c_int64(-1)
    want = {0: n * T * 10 * 14 * 64, 1: n * T * 128, 2: n * T * 128, 3: n * T * 4 * hidden, 4: n * T * hidden, 5: n * T * hidden}
    for stage, elems in want.items():                       # dst == NULL reports the count (before any run, too)
        assert fn(plan.handle, stage, n, None, 0, C.byref(count), st) == N.RVA_OK and count.value == elems
    plan.run(ring, iota, n)
    dst = torch.full((want[0] + 8,), -7.0, dtype=torch.float16, device=DEV)
    ptr = C.c_void_p(dst.data_ptr())
    for bad in ((6, n, ptr, dst.numel()), (-1, n, ptr, dst.numel()), (0, n, ptr, want[0] - 1), (0, cap + 1, ptr, 1 << 30),
                (0, 0, ptr, dst.numel())):
        assert fn(plan.handle, *bad, None, st) == N.RVA_ERR_ARG, bad
    assert fn(None, 0, n, ptr, dst.numel(), None, st) == N.RVA_ERR_ARG
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())                        # a refused call copies nothing
    assert fn(plan.handle, 0, n, ptr, dst.numel(), C.byref(count), st) == N.RVA_OK and count.value == want[0]
    assert torch.equal(dst[:want[0]].view(n * T, 10, 14, 64), plan.stage("pooled", n)) and bool((dst[want[0]:] == -7.0).all())
    with pytest.raises(ValueError, match="unknown stage"):
        plan.stage("conv2", n)
    with pytest.raises(RuntimeError, match="capacity"):
        plan.stage("feat", cap + 1)
