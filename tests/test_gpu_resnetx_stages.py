"""Every stage of the any-depth fp16 ResNet plan (resnet_plan.FusedResNetF16, ``rva_resnetx_f16_plan_*`` in
csrc/rva_resnet_f16.hip) against float64 on the GPU, through the workspace tap: ``pooled``, each block's inner convolutions, the
shortcut convolutions of split plans, each block's output -- for fused plans the launch that carries the shortcut convolution in
its own sum --, the mean over 512 or 2048 channels and the logits.  Each reference is computed from the tap(s) the launch itself
read, with the bounds of tests/resnetx_refs.py, so a failure names the launch.

Cases: Bottleneck (1,2,1,1) at 5 x 40 x 72 (non-square maps 10 x 18 .. 2 x 3, an identity block, every shortcut kind: stride 1
with 64 input channels, stride 2 with 256 / 512 / 1024), BasicBlock (2,2,2,2) at 4 x 33 x 47 (odd maps 9 x 12, 5 x 6, 3 x 3, 2 x 2:
tiles that span images, M not a multiple of 32) and ResNet-50 at 3 x 64 x 64; each as a fused and as a split plan.  Then the
cross-check against the verified ResNet-18 plan: a ``classify.ResNet`` carrying a ``classify.ResNet18``'s weights, run split, must
leave the bits of ``FusedResNet18F16``.

Observed / bound: printed per stage kind (``pytest -s``)."""
import ctypes as C

import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops, synth
from realtime_video_analytics_32streams_amd.classify import ResNet, ResNet18
from realtime_video_analytics_32streams_amd.resnet_plan import FusedResNet18F16, FusedResNetF16, resnet_maps
from tests import resnetx_refs as X

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
STAGE_CASES = (X.SMALL_BOTT, X.SMALL_BASIC, X.RESNET50)


def _run(plan, frames, index, n):
    logits = plan.run(frames, index, n).clone()
    taps = {k: plan.stage(k, n) for k in plan.stage_names}
    taps["logits"] = logits
    return taps


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "split"])
@pytest.mark.parametrize("case", STAGE_CASES, ids=X.case_id)
def test_every_stage_against_float64(case, fused):
    block, blocks, B, H, W, classes = case[:6]
    bott = block == "bottleneck"
    net, p, frames16 = X.stage_case(case, fused)
    plan = FusedResNetF16(net, (H, W), B + 1, split_shortcut=not fused)          # a capacity above the batch
    names = X.stage_names(bott, blocks, fused)
    n_short = sum(t["shortcut"] for t in X.layout(bott, blocks))
    assert plan.stage_names == names and plan.maps == resnet_maps(H, W)
    assert plan.n_launches == 1 + sum(blocks) * (3 if bott else 2) + (0 if fused else n_short) + 2
    taps = _run(plan, frames16.to(DEV).contiguous(), torch.arange(B, dtype=torch.int32, device=DEV), B)
    f16 = set(X.f16_stages(bott, blocks, fused))
    for k in names + ("logits",):
        assert taps[k].dtype == (torch.float16 if k in f16 else torch.float32), k
    assert tuple(taps[names[-2]].shape) == (B, *plan.maps[4], 512 * net.expansion) and tuple(taps["logits"].shape) == (B, classes)
    assert tuple(taps["feat"].shape) == (B, 512 * net.expansion)
    refs = X.refsx({k: v.cpu() for k, v in taps.items()}, frames16, p, bott, blocks, fused)
    bad, worst = [], {}
    for k in names + ("logits",):
        got, (ref, tol) = taps[k].cpu(), refs[k]
        assert tuple(got.shape) == tuple(ref.shape), (k, tuple(got.shape), tuple(ref.shape))
        r, e = X.R.ratio(got, ref, tol)
        kind = k.split(".")[-1]
        worst[kind] = max(worst.get(kind, 0.0), r)
        if not r <= 1.0:
            bad.append(f"{k}: observed / bound = {r:.3f} (max err {e:.3e})")
    print(f"{X.case_id(case)} {'fused' if fused else 'split'}: observed / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not bad, bad
    assert all(bool((taps[k] != 0).any()) for k in names)


@pytest.mark.parametrize("hw", [(34, 34), (40, 72)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_a_split_plan_with_resnet18s_weights_leaves_the_resnet18_plans_bits(hw):
    """The same kernels in the same order on the same weights: logits and every block output are bit-identical.  Both sides now
    run the one plan of csrc/rva_resnet_f16.hip (``rva_resnet_f16_plan_*`` creates it with the ResNet-18 descriptor), so this
    checks the two front doors -- the packers, the descriptor and the stage-code translation -- against each other; that the bits
    are still those of the separate ResNet-18 plan was shown when it was deleted (profiles/resnet_one_topology.json)."""
    old = synth.seeded_module(lambda: ResNet18(10), 77)
    new = ResNet("basic", (2, 2, 2, 2), 10)
    sd = {"conv1.weight": old.stem[0].weight, **{f"bn1.{k}": v for k, v in old.stem[1].state_dict().items()},
          "fc.weight": old.fc.weight, "fc.bias": old.fc.bias}
    for b, blk in enumerate(old.layers):
        pre = f"layer{b // 2 + 1}.{b % 2}."
        sd[pre + "conv1.weight"], sd[pre + "conv2.weight"] = blk.c1.weight, blk.c2.weight
        sd.update({f"{pre}bn1.{k}": v for k, v in blk.b1.state_dict().items()})
        sd.update({f"{pre}bn2.{k}": v for k, v in blk.b2.state_dict().items()})
        if blk.down is not None:
            sd[pre + "downsample.0.weight"] = blk.down[0].weight
            sd.update({f"{pre}downsample.1.{k}": v for k, v in blk.down[1].state_dict().items()})
    new.load_state_dict(sd, strict=True)
    new.eval()
    B = 5
    x = synth.seeded_clip((B, 3, *hw), 78).half().to(DEV).contiguous()
    iota = torch.arange(B, dtype=torch.int32, device=DEV)
    ref, got = FusedResNet18F16(old, hw, B), FusedResNetF16(new, hw, B, split_shortcut=True)
    assert got.n_launches == ref.n_launches == 22 and got.workspace_bytes == ref.workspace_bytes
    want = ref.run(x, iota, B).clone()
    have = got.run(x, iota, B).clone()
    assert torch.equal(have, want) and bool((want != 0).any())
    assert torch.equal(got.stage("pooled", B), ref.stage("pooled", B)) and torch.equal(got.stage("feat", B), ref.stage("feat", B))
    for b in range(8):
        assert torch.equal(got.stage(f"b{b}.out", B), ref.stage(f"out{b}", B)), b
        assert torch.equal(got.stage(f"b{b}.mid1", B), ref.stage(f"mid{b}", B)), b
    for b in (2, 4, 6):
        assert torch.equal(got.stage(f"b{b}.down", B), ref.stage(f"down{b}", B)), b
    assert FusedResNetF16(new, hw, B).n_launches == 19       # the default plan: the three shortcut convolutions have no launch


def test_tap_contract_and_stages_the_plan_lacks():
    case = X.SMALL_BOTT
    block, blocks, B, H, W, classes = case[:6]                # maps 10 x 18, 5 x 9, 3 x 5, 2 x 3
    net, p, frames16 = X.stage_case(case, True)
    cap = B + 2
    fused, split = FusedResNetF16(net, (H, W), cap), FusedResNetF16(net, (H, W), cap, split_shortcut=True)
    assert split.workspace_bytes - fused.workspace_bytes == cap * 2 * (180 * 256 + 45 * 512 + 15 * 1024 + 6 * 2048)
    fn, st = fused.L.rva_resnetx_f16_plan_stage, ops._stream_ptr()
    count = C.c_int64(-1)
    code = lambda b, slot: N.RVA_RESX_BLOCK0 + 4 * b + slot  # noqa: E731
    want = {N.RVA_RESX_POOLED: B * 180 * 64, N.RVA_RESX_FEAT: B * 2048, code(0, 0): B * 180 * 64, code(0, 1): B * 180 * 64,
            code(0, 3): B * 180 * 256, code(1, 0): B * 180 * 128, code(1, 1): B * 45 * 128, code(1, 3): B * 45 * 512,
            code(2, 3): B * 45 * 512, code(4, 3): B * 6 * 2048}
    for stage, elems in want.items():                         # dst == NULL reports the count (before any run, too)
        assert fn(fused.handle, stage, B, None, 0, C.byref(count), st) == N.RVA_OK and count.value == elems, stage
    for plan, lacks in ((fused, [code(0, 2), code(1, 2), code(2, 2)]), (split, [code(2, 2)])):
        for stage in lacks + [-1, code(5, 0), code(4, 3) + 1]:
            assert fn(plan.handle, stage, B, None, 0, C.byref(count), st) == N.RVA_ERR_ARG, stage
            assert b"no stage" in N.lib().rva_last_error(plan.ctx.handle)
    assert fn(split.handle, code(0, 2), B, None, 0, C.byref(count), st) == N.RVA_OK and count.value == B * 180 * 256
    x = frames16.to(DEV).contiguous()
    fused.run(x, torch.arange(B, dtype=torch.int32, device=DEV), B)
    for stage, dtype, name in ((code(3, 3), torch.float16, "b3.out"), (code(4, 3), torch.float32, "b4.out"), (N.RVA_RESX_FEAT, torch.float32, "feat")):
        n_el = int(fused.stage(name, B).numel())
        dst = torch.full((n_el + 8,), -7.0, dtype=dtype, device=DEV)
        ptr = C.c_void_p(dst.data_ptr())
        for bad in ((stage, B, ptr, n_el - 1), (stage, cap + 1, ptr, 1 << 30), (stage, 0, ptr, dst.numel())):
            assert fn(fused.handle, *bad, None, st) == N.RVA_ERR_ARG, bad
        assert fn(None, stage, B, ptr, dst.numel(), None, st) == N.RVA_ERR_ARG
        torch.cuda.synchronize()
        assert bool((dst == -7.0).all())                     # a refused call copies nothing
        assert fn(fused.handle, stage, B, ptr, dst.numel(), C.byref(count), st) == N.RVA_OK and count.value == n_el
        got = fused.stage(name, B)
        assert got.dtype == dtype and torch.equal(dst[:n_el].view(got.shape), got) and bool((dst[n_el:] == -7.0).all())
    with pytest.raises(ValueError, match="unknown stage"):
        fused.stage("b0.down", B)
    with pytest.raises(ValueError, match="unknown stage"):
        split.stage("b2.down", B)                             # an identity block has no shortcut convolution
    with pytest.raises(RuntimeError, match="capacity"):
        fused.stage("feat", cap + 1)
