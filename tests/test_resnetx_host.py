"""CPU-only checks of the any-depth ResNet head (classify.ResNet, classify.build_resnet, resnet_plan.pack_resnet /
resnet_any_flops, the detector's routing by ``model_path``) and of the constants of tests/resnetx_refs.py: the per-case tolerances
are 4 x what the float64 emulation measures, the stored activations stay far inside fp16's range, and the top-6 gaps leave at most
one frame per case out of the top-5 comparison."""
import copy
import math

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import classify as CL
from realtime_video_analytics_32streams_amd import resnet_plan as RP
from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.clip_plan import _fold64
from realtime_video_analytics_32streams_amd.config import DetectorConfig
from tests import resnetx_refs as X

BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
BASIC_KEYS = ["conv1.weight"] + [f"bn1.{a}" for a in BN] + ["conv2.weight"] + [f"bn2.{a}" for a in BN]
BOTT_KEYS = BASIC_KEYS + ["conv3.weight"] + [f"bn3.{a}" for a in BN]
DOWN_KEYS = ["downsample.0.weight"] + [f"downsample.1.{a}" for a in BN]
PARAMS = {18: 11_689_512, 34: 21_797_672, 50: 25_557_032, 101: 44_549_160, 152: 60_192_808}


def _torchvision_keys(depth):
    block, blocks = CL.RESNET_DEPTHS[depth]
    keys = ["conv1.weight"] + [f"bn1.{a}" for a in BN]
    for s, n in enumerate(blocks):
        for j in range(n):
            down = j == 0 and (s > 0 or block == "bottleneck")
            keys += [f"layer{s + 1}.{j}.{k}" for k in (BOTT_KEYS if block == "bottleneck" else BASIC_KEYS) + (DOWN_KEYS if down else [])]
    return keys + ["fc.weight", "fc.bias"]


# ---------------------------------------------------------------------------------------------------------------------
# module and loader
@pytest.mark.parametrize("depth", sorted(PARAMS))
def test_state_dict_keys_and_parameter_counts_are_torchvisions(depth):
    block, blocks = CL.RESNET_DEPTHS[depth]
    net = CL.ResNet(block, blocks, 1000)
    assert list(net.state_dict()) == _torchvision_keys(depth)
    assert sum(p.numel() for p in net.parameters()) == PARAMS[depth]
    assert CL.resnet_depth_of(net) == depth and net.fc.in_features == 512 * net.expansion
    if block == "basic":
        assert net.layer1[0].downsample is None and net.layer2[0].downsample[0].stride == (2, 2)
    else:                                     # the first block of layer1 has a stride-1 shortcut convolution
        d = net.layer1[0].downsample[0]
        assert (d.in_channels, d.out_channels, d.stride) == (64, 256, (1, 1))
        assert net.layer2[0].conv2.stride == (2, 2) and net.layer2[0].conv1.stride == (1, 1)      # the stride is on the 3x3
    with torch.inference_mode():
        assert tuple(net.eval()(torch.zeros(1, 3, 33, 47)).shape) == (1, 1000)


def test_module_refuses_what_is_outside_the_family():
    with pytest.raises(ValueError, match="basic"):
        CL.ResNet("resnext", (3, 4, 6, 3))
    for blocks in ((3, 4, 6), (0, 1, 1, 1), (1, 1, 65, 1)):
        with pytest.raises(ValueError, match="1..64"):
            CL.ResNet("basic", blocks)


@pytest.mark.parametrize("prefix", ["", "module.", "model."])
@pytest.mark.parametrize("block,blocks,classes", [("basic", (2, 2, 2, 2), 7), ("bottleneck", (1, 2, 1, 1), 12), ("basic", (1, 3, 1, 2), 5)])
def test_loader_round_trip(tmp_path, prefix, block, blocks, classes):
    net = synth.seeded_module(lambda: CL.ResNet(block, blocks, classes), 17)
    path = tmp_path / "anything.pt"
    torch.save({prefix + k: v for k, v in net.state_dict().items()}, path)
    got = CL.build_resnet(weights=str(path))
    assert (got.block, got.blocks, got.fc.out_features) == (block, tuple(blocks), classes) and not got.training
    assert synth.state_sha(got.state_dict()) == synth.state_sha(net.state_dict())
    x = synth.seeded_clip((2, 3, 40, 40), 3)
    with torch.inference_mode():
        assert torch.equal(got(x), net(x))
    assert CL.build_resnet(weights=str(path), num_classes=classes).fc.out_features == classes
    # a checkpoint wrapper, and a state dict without num_batches_tracked
    torch.save({"state_dict": {k: v for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}}, path)
    assert synth.state_sha(CL.build_resnet(weights=str(path)).state_dict()) == synth.state_sha(net.state_dict())


def test_seeded_build_is_reproducible_and_leaves_the_global_generator_alone():
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    a, b = CL.build_resnet(34, seed=4, num_classes=9), CL.build_resnet(34, seed=4, num_classes=9)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert synth.state_sha(a.state_dict()) == synth.state_sha(b.state_dict()) != synth.state_sha(CL.build_resnet(34, seed=5, num_classes=9).state_dict())
    assert CL.resnet_depth_of(a) == 34 and a.fc.out_features == 9 and CL.build_resnet(50).fc.out_features == 1000
    assert float(a.bn1.running_var.std()) > 0                              # non-trivial statistics: the fold is not a no-op
    with pytest.raises(ValueError, match="depth"):
        CL.build_resnet(20)
    with pytest.raises(ValueError, match="depth"):
        CL.build_resnet(weights="/nonexistent/resnet50.pt")             # no file and no depth: nothing is fetched by name


def _save(tmp_path, sd):
    path = tmp_path / "net.pt"
    torch.save(sd, path)
    return str(path)


def test_loader_refusals_name_the_key_and_the_shape(tmp_path):
    net = CL.ResNet("bottleneck", (1, 1, 1, 1), 10)
    sd = net.state_dict()

    def refused(change, match):
        bad = {k: v.clone() for k, v in sd.items()}
        change(bad)
        with pytest.raises(ValueError, match=match):
            CL.build_resnet(weights=_save(tmp_path, bad))

    def resnext(d):                                                       # groups = 32, width 128: conv2 [128, 4, 3, 3]
        d["layer1.0.conv1.weight"] = torch.zeros(128, 64, 1, 1)
        d["layer1.0.conv2.weight"] = torch.zeros(128, 4, 3, 3)
    refused(resnext, r"layer1\.0\.conv2\.weight is \(128, 4, 3, 3\).*grouped")

    def wide(d):                                                          # wide_resnet50_2: width 128 in layer1
        d["layer1.0.conv1.weight"] = torch.zeros(128, 64, 1, 1)
        d["layer1.0.conv2.weight"] = torch.zeros(128, 128, 3, 3)
    refused(wide, r"layer1\.0\.conv1\.weight is \(128, 64, 1, 1\).*wide")

    refused(lambda d: d.update({"conv1.weight": torch.zeros(64, 3, 3, 3)}), r"conv1\.weight is \(64, 3, 3, 3\).*7x7 / 64")
    refused(lambda d: d.update({"conv1.weight": torch.zeros(32, 3, 7, 7)}), r"conv1\.weight is \(32, 3, 7, 7\).*7x7 / 64")
    refused(lambda d: d.pop("layer2.0.bn2.running_var"), r"layer2\.0\.bn2\.weight of shape \(128,\) has no layer2\.0\.bn2\.running_var")
    refused(lambda d: d.pop("bn1.running_mean"), r"bn1\.weight of shape \(64,\) has no bn1\.running_mean")
    refused(lambda d: d.pop("fc.weight"), r"no 'fc\.weight'")
    path = _save(tmp_path, sd)
    with pytest.raises(ValueError, match=r"fc\.weight is \(10, 2048\).*10 classes.*resnet_num_classes says 1000"):
        CL.build_resnet(weights=path, num_classes=1000)
    with pytest.raises(ValueError, match="state dict of tensors"):
        CL.build_resnet(weights=_save(tmp_path, [1, 2, 3]))


# ---------------------------------------------------------------------------------------------------------------------
# packer and FLOP counts
def _pairs(net):
    out = []
    for s in range(4):
        for blk in getattr(net, f"layer{s + 1}"):
            own = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)] + ([(blk.conv3, blk.bn3)] if net.block == "bottleneck" else [])
            out.append((own, None if blk.downsample is None else (blk.downsample[0], blk.downsample[1])))
    return out


@pytest.mark.parametrize("block,blocks", [("bottleneck", (1, 2, 1, 1)), ("basic", (2, 2, 2, 2)), ("basic", (1, 1, 1, 1))])
def test_pack_order_shapes_roundings_and_the_fused_bias(block, blocks):
    net = synth.seeded_module(lambda: CL.ResNet(block, blocks, 11), 23)
    fused, split = RP.pack_resnet(net), RP.pack_resnet(net, fused=False)
    n = X.n_convs(fused)
    assert list(fused) == list(split) == ["stem_w", "stem_b"] + [f"c{i}_{x}" for i in range(n) for x in "wb"] + ["head_w", "head_b"]
    assert all(v.dtype == np.float32 and v.flags.c_contiguous for v in fused.values())
    assert fused["stem_w"].shape == (64, 3, 7, 7) and fused["head_w"].shape == (11, 512 * net.expansion)
    i, n_short = 0, 0
    for own, short in _pairs(net):
        biases = []
        for conv, bn in own + ([short] if short else []):
            w64, b64 = _fold64(conv, bn)
            want = w64.numpy().astype(np.float16).astype(np.float32)                      # float64 -> fp16: one rounding
            want = want.reshape(want.shape[0], want.shape[1], -1).transpose(0, 2, 1)      # [co, k*k, ci]
            assert np.array_equal(fused[f"c{i}_w"], want) and np.array_equal(split[f"c{i}_w"], want), i
            assert fused[f"c{i}_w"].shape == (conv.out_channels, conv.kernel_size[0] ** 2, conv.in_channels)
            assert np.array_equal(split[f"c{i}_b"], b64.float().numpy()), i
            biases.append((i, b64))
            i += 1
        if short:
            n_short += 1
            (ic, bc), (is_, bs) = biases[-2], biases[-1]
            assert np.array_equal(fused[f"c{ic}_b"], (bc + bs).float().numpy())           # the float64 sum rounded once
            assert np.array_equal(fused[f"c{is_}_b"], bs.float().numpy())
            biases = biases[:-2]
        for j, b64 in biases:
            assert np.array_equal(fused[f"c{j}_b"], b64.float().numpy()), j
    assert i == n and n_short == sum(t["shortcut"] for t in RP.resnet_blocks(block == "bottleneck", blocks)) >= 3
    assert not np.array_equal(RP.pack_resnet(net, half=False)["c0_w"], fused["c0_w"])


def test_pack_refusals():
    net = synth.seeded_module(lambda: CL.ResNet("bottleneck", (1, 1, 1, 1), 5), 29)
    names = {"stem_w": "conv1.weight", "c0_w": "layer1.0.conv1.weight", "c3_w": "layer1.0.downsample.0.weight",
             "c9_w": "layer3.0.conv2.weight"}
    for name, key in names.items():
        big = copy.deepcopy(net)
        with torch.no_grad():
            dict(big.named_parameters())[key].view(-1)[5] = 1e6
        with pytest.raises(ValueError, match=f"pack_resnet: a value of {name} does not stay finite"):
            RP.pack_resnet(big)
        RP.pack_resnet(big, half=False)
    with pytest.raises(ValueError, match="not a classify.ResNet.*ResNet18"):
        RP.pack_resnet(CL.ResNet18(5))
    with pytest.raises(ValueError, match="not a classify.ResNet"):
        RP.pack_resnet(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="not the ResNet18 architecture"):               # and the ResNet-18 packer keeps its own
        RP.pack_resnet18(CL.ResNet("basic", (2, 2, 2, 2), 5))


def test_flop_counts_follow_the_formulas():
    f = RP.resnet_any_flops(True, (3, 4, 6, 3), 224, 224, 1000)
    assert f["stem"] == 2.0 * 112 * 112 * 64 * 147 and f["head"] == 2.0 * 2048 * 1000
    assert len(f["launches"]) == 48 and len(RP.resnet_any_flops(True, (3, 4, 6, 3), 224, 224, split_shortcut=True)["launches"]) == 52
    by = {n: (fl, by_, px, K, co) for n, fl, by_, px, K, co in f["launches"]}
    assert by["b0.mid1"] == (2.0 * 3136 * 64 * 64, 2.0 * (3136 * 64 + 64 * 64) + 2 * 3136 * 64, 3136, 64, 64)
    assert by["b0.out"][3:] == (64 + 64, 256) and by["b0.out"][0] == 2.0 * 3136 * 256 * 128
    assert by["b3.mid1"][2:] == (3136, 256, 128) and by["b3.mid2"][2:] == (784, 9 * 128, 128)   # the stride is on the 3x3
    assert by["b3.out"][3:] == (128 + 256, 512) and by["b4.out"][3:] == (128, 512)
    assert by["b15.out"][1] == 2.0 * (49 * 512 + 512 * 2048) + 4 * 49 * 2048 + 2.0 * 49 * 2048    # fp32 out, fp16 residual
    assert 8.0e9 < f["frame"] < 8.4e9                                       # 4.1 G multiply-adds: the published ResNet-50 figure
    split = RP.resnet_any_flops(True, (3, 4, 6, 3), 224, 224, split_shortcut=True)
    assert split["frame"] == f["frame"]
    # what the fused form saves per frame: the four `down` tensors, written and read back
    down = 2 * (3136 * 256 + 784 * 512 + 196 * 1024 + 49 * 2048)
    assert split["workspace_bytes"] - f["workspace_bytes"] == down and 2.9e6 < down < 3.1e6
    g = RP.resnet_any_flops(False, (2, 2, 2, 2), 224, 224, 1000, split_shortcut=True)
    r18 = RP.resnet_flops(224, 224, 1000)
    assert g["frame"] == r18["frame"] and [c[1] for c in g["launches"]] == [c[1] for c in r18["convs"]]


# ---------------------------------------------------------------------------------------------------------------------
# the end-to-end constants
def _up2(v):
    e = 10.0 ** (math.floor(math.log10(v)) - 1)
    return math.ceil(v / e - 1e-9) * e


@pytest.mark.parametrize("case", X.E2E_CASES, ids=X.case_id)
def test_emulation_defines_the_tolerances_and_the_gaps_hold(case):
    c = X.e2e(case)
    dq, do = float(np.abs(c["emu"] - c["quant"]).max()), float(np.abs(c["emu"] - c["orig"]).max())
    ds = float(np.abs(c["emu_split"] - c["quant"]).max())
    gaps = X.top_gaps(c["quant"])
    print(f"    {X.case_id(case):44s} {dq:.3e}          {do:.3e}         {ds:.3e}                 "
          f"{sum(g > 2 * _up2(4 * dq) for g in gaps)} of {len(gaps)}        {' '.join(f'{g:.1e}' for g in gaps)}   peak {c['peak']:.2f}")
    print(f"    TOL_Q = {_up2(4 * dq):.2e}, TOL_O = {_up2(4 * do):.2e}")
    assert c["peak"] < 1e3                                                   # far inside fp16's range
    # rounding up to two digits adds less than 10 %
    assert 4 * dq <= X.TOL_Q[case] <= 1.1 * 4 * dq
    assert 4 * do <= X.TOL_O[case] <= 1.1 * 4 * do
    clear = X.clear_frames(case, c["quant"])
    assert len(clear) - sum(clear) <= X.LEAVE_OUT
    for e, s, q, ok in zip(c["emu"], c["emu_split"], c["quant"], clear):
        if ok:
            assert X.top(e).tolist() == X.top(q).tolist() == X.top(s).tolist()


@pytest.mark.parametrize("case,fused", [(X.SMALL_BOTT, True), (X.SMALL_BOTT, False), (X.SMALL_BASIC, True), (X.SMALL_BASIC, False)],
                         ids=lambda v: X.case_id(v) if isinstance(v, tuple) else ("fused" if v else "split"))
def test_float64_chain_rounded_to_the_storage_types_is_inside_every_bound(case, fused):
    """The references alone meet what the GPU stage test imposes, and the bounds see a fused launch that forgets the shortcut."""
    bott, blocks = case[0] == "bottleneck", case[1]
    net, p, x16 = X.stage_case(case, fused)
    refs = X.refsx(None, x16, p, bott, blocks, fused)
    names = X.stage_names(bott, blocks, fused)
    f16 = set(X.f16_stages(bott, blocks, fused))
    assert set(refs) == set(names) | {"logits"}
    taps = {k: (X.R.f64(v[0]).half() if k in f16 else X.R.f64(v[0]).float()) for k, v in refs.items()}
    again = X.refsx(taps, x16, p, bott, blocks, fused)
    bad = []
    for k in names + ("logits",):
        X.R.report(case[2:6], k, taps[k], *again[k], out=bad)
    assert not bad, bad
    if fused:                                     # the sum without the shortcut's channels leaves the bound by far more than 4 x
        lay = X.layout(bott, blocks)
        b = next(i for i, t in enumerate(lay) if t["shortcut"])
        t = lay[b]
        close = t["convs"][-1]
        a = X.R.nchw(taps[f"b{b}.mid2" if bott else f"b{b}.mid1"])
        y = torch.nn.functional.conv2d(a, p[f"c{close}_w"], p[f"c{close}_b"], padding=0 if bott else 1).relu()
        assert X.R.ratio(X.R.nhwc(y).half(), *again[f"b{b}.out"])[0] > 4.0


# ---------------------------------------------------------------------------------------------------------------------
# detector routing (the device is not touched before a plan is made: a fake context stands in for it)
class _FakeCtx:
    device = 0


def _dcfg(**kw):
    base = dict(model_path="resnet50.pt", backend="hip", model_type="resnet", confidence_threshold=-1e9, resnet_num_classes=10,
                resnet_top_k=3, input_size=[64, 64], warmup=False, half=True, hip_engine="plan", hip_resnet_fp16=True)
    base.update(kw)
    return DetectorConfig(**base)


@pytest.fixture
def cpu_detector(monkeypatch):
    """``HipResNetDetector`` built without a GPU: the context is faked and the module stays on the CPU."""
    monkeypatch.setattr(CL.ops, "context", lambda device=None: _FakeCtx())
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)

    def make(**kw):
        net = kw.pop("net", None)
        return CL.HipResNetDetector(_dcfg(**kw), net=net)
    return make


def _seeded_resnet18(classes, seed=2):
    st = torch.random.get_rng_state()
    torch.manual_seed(seed)
    net = CL.ResNet18(classes)
    torch.random.set_rng_state(st)
    return net


def test_routing_by_name_without_a_file(cpu_detector):
    for name, depth in (("resnet50.pt", 50), ("ResNet34.onnx", 34), ("models/RESNET101_v2.xml", 101), ("resnet152", 152)):
        d = cpu_detector(model_path=name)
        assert type(d.net) is CL.ResNet and CL.resnet_depth_of(d.net) == depth and d.engine == "resnet-f16", name
        assert d.net.fc.out_features == 10 and not d.net.training
        assert synth.state_sha(d.net.state_dict()) == synth.state_sha(CL.build_resnet(depth, seed=2, num_classes=10).state_dict())
    want = synth.state_sha(_seeded_resnet18(10).state_dict())
    for name in ("resnet.onnx", "resnet18.onnx", "resnet18.pt", "classifier.xml", "myresnet50.pt"):       # today's seeded ResNet-18
        for kw in (dict(), dict(half=False), dict(hip_engine="auto")):
            d = cpu_detector(model_path=name, **kw)
            assert type(d.net) is CL.ResNet18 and synth.state_sha(d.net.state_dict()) == want, (name, kw)
    assert cpu_detector(model_path="resnet.onnx", half=False).engine == "resnet-f32"
    assert CL.resnet_depth_from_path("/a/b/ResNet50-int8.xml") == 50 and CL.resnet_depth_from_path("resnet5.pt") is None


def test_routing_by_an_existing_state_dict(cpu_detector, tmp_path):
    for block, blocks, name in (("bottleneck", (1, 2, 1, 1), "whatever.pt"), ("basic", (2, 2, 2, 2), "resnet18.pt"),
                                ("basic", (1, 1, 2, 1), "resnet50.pt")):
        net = synth.seeded_module(lambda: CL.ResNet(block, blocks, 10), 31)
        path = tmp_path / name
        torch.save({"module." + k: v for k, v in net.state_dict().items()}, path)
        d = cpu_detector(model_path=str(path))                                 # what the file says, whatever its name
        assert type(d.net) is CL.ResNet and (d.net.block, d.net.blocks) == (block, blocks) and d.engine == "resnet-f16"
        assert synth.state_sha(d.net.state_dict()) == synth.state_sha(net.state_dict())
    given = CL.ResNet18(10)
    assert cpu_detector(model_path=str(path), net=given).net is given           # net=... overrides the file
    assert cpu_detector(model_path=str(path), hip_engine="auto").engine == "torch"
    with pytest.raises(ValueError, match=r"fc\.weight is \(10, 512\).*resnet_num_classes says 1000"):       # the detector hands the key over
        cpu_detector(model_path=str(path), resnet_num_classes=1000)


def test_the_fp32_plan_is_refused_for_the_general_module_at_construction(cpu_detector):
    for kw in (dict(half=False), dict(hip_resnet_fp16=False), dict(half=False, hip_resnet_fp16=False)):
        for extra in (dict(), dict(net=CL.ResNet("basic", (1, 1, 1, 1), 10))):
            with pytest.raises(ValueError) as e:
                cpu_detector(**kw, **extra)
            msg = str(e.value)
            assert "resnet-f32" in msg and "classify.ResNet18 only" in msg
            assert "half: true" in msg and "hip_resnet_fp16: true" in msg and "hip_engine: auto" in msg        # both ways out
    for kw in (dict(half=False), dict(half=True), dict(hip_resnet_fp16=False)):     # auto: PyTorch-ROCm fp32, as for ResNet-18
        d = cpu_detector(hip_engine="auto", **kw)
        assert d.engine == "torch" and type(d.net) is CL.ResNet and next(d.net.parameters()).dtype == torch.float32
    with pytest.raises(ValueError, match="no hand-written plan"):                # native without the fp16 key: as before
        cpu_detector(hip_engine="native", half=False)
    assert cpu_detector(hip_engine="native").engine == "resnet-f16"


def test_the_six_entries_are_exported_with_the_resnet18_plans_signatures():
    names = ["rva_resnetx_f16_plan_" + n for n in ("create", "destroy", "info", "run", "run_post", "stage")]
    assert all(n in N.EXPORTS for n in names)
    assert RP.FusedResNetF16.ABI == "rva_resnetx_f16_plan" and RP.FusedResNetF16.RING_DTYPE == torch.float16
    for n in ("destroy", "info", "run", "run_post", "stage"):
        new, old = getattr(N.lib(), f"rva_resnetx_f16_plan_{n}"), getattr(N.lib(), f"rva_resnet_f16_plan_{n}")
        assert new.argtypes == old.argtypes and new.restype == old.restype, n
    assert [f[0] for f in N.ResNetXDesc._fields_] == ["height", "width", "classes", "top_k", "max_frames", "bottleneck", "blocks",
                                                      "n_convs", "flags"]
    assert (N.RVA_RESX_SPLIT_SHORTCUT, N.RVA_RESX_POOLED, N.RVA_RESX_FEAT, N.RVA_RESX_BLOCK0) == (1, 0, 1, 2)
