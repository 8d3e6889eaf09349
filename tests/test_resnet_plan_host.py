"""CPU-side checks of the fp32 ResNet-18 plan's host pieces (resnet_plan.py): the packer folds BatchNorm into the ABI's weight
layout and refuses other architectures, the FLOP count follows its formulas, and the binding exports the plan's entry points."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import resnet_plan as RP
from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.classify import ResNet18


def _forward_packed(p, x):
    """The network from the packed arrays alone (float64)."""
    t = {k: torch.from_numpy(v).double() for k, v in p.items()}
    conv = lambda i, x, s, pad: F.conv2d(x, t[f"c{i}_w"].permute(0, 2, 1).reshape(  # noqa: E731
        t[f"c{i}_w"].shape[0], t[f"c{i}_w"].shape[2], *([int(round(t[f"c{i}_w"].shape[1] ** 0.5))] * 2)), t[f"c{i}_b"], stride=s, padding=pad)
    x = F.max_pool2d(F.conv2d(x.double(), t["stem_w"], t["stem_b"], stride=2, padding=3).relu(), 3, 2, 1)
    i = 0
    for cin, c, s in RP.block_shapes():
        y = conv(i + 1, conv(i, x, s, 1).relu(), 1, 1)
        r = conv(i + 2, x, 2, 0) if cin != c else x
        i += 3 if cin != c else 2
        x = (y + r).relu()
    assert i == 19
    return x.mean((2, 3)) @ t["head_w"].T + t["head_b"]


def test_packer_folds_batchnorm_in_the_abi_layout():
    net = synth.seeded_module(lambda: ResNet18(23), 7)
    p = RP.pack_resnet18(net)
    assert tuple(p) == N.ResNetWeights.NAMES and len(N.ResNetWeights.NAMES) == 2 + 2 * 19 + 2
    assert all(v.dtype == np.float32 and v.flags["C_CONTIGUOUS"] for v in p.values())
    assert p["stem_w"].shape == (64, 3, 7, 7) and p["head_w"].shape == (23, 512) and p["head_b"].shape == (23,)
    shapes = [p[f"c{i}_w"].shape for i in range(19)]
    assert shapes[:4] == [(64, 9, 64)] * 4 and shapes[4:7] == [(128, 9, 64), (128, 9, 128), (128, 1, 64)]
    assert shapes[11] == (256, 1, 128) and shapes[16] == (512, 1, 256) and shapes[18] == (512, 9, 512)
    assert all(p[f"c{i}_b"].shape == (shapes[i][0],) for i in range(19))
    x = synth.seeded_clip((2, 3, 40, 56), 3)
    with torch.no_grad():
        want = net.double()(x.double())
    got = _forward_packed(p, x)
    assert float((got - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


def test_packer_refuses_other_architectures():
    net = ResNet18(10)
    net.fc = torch.nn.Linear(256, 10)
    with pytest.raises(ValueError, match="pack_resnet18: not the ResNet18 architecture"):
        RP.pack_resnet18(net)
    net = ResNet18(10)
    net.layers[2].c1 = torch.nn.Conv2d(64, 128, 3, 1, 1, bias=False)         # the first 128-wide block without its stride
    with pytest.raises(ValueError, match="not the ResNet18 architecture"):
        RP.pack_resnet18(net)
    net = ResNet18(10)
    net.stem[3] = torch.nn.MaxPool2d(2, 2)
    with pytest.raises(ValueError, match="not the ResNet18 architecture"):
        RP.pack_resnet18(net)
    with pytest.raises(ValueError, match="not the ResNet18 architecture"):
        RP.pack_resnet18(torch.nn.Linear(3, 3))
    seq = ResNet18(10)
    seq.layers = torch.nn.Sequential(*list(seq.layers)[:6])
    with pytest.raises(ValueError, match="not the ResNet18 architecture"):
        RP.pack_resnet18(seq)


def test_flops_follow_the_formulas():
    f = RP.resnet_flops(224, 224, 1000)
    assert f["stem"] == 2.0 * 112 * 112 * 64 * 147
    convs = {n: (fl, px, k, c) for n, fl, px, k, c in f["convs"]}
    assert len(f["convs"]) == 19 and [c[0] for c in f["convs"]][4:7] == ["mid2", "down2", "out2"]
    assert convs["mid0"] == (2.0 * 56 * 56 * 64 * 576, 3136, 576, 64)
    assert convs["mid2"] == (2.0 * 28 * 28 * 128 * 576, 784, 576, 128) and convs["down2"] == (2.0 * 784 * 128 * 64, 784, 64, 128)
    assert convs["out7"] == (2.0 * 49 * 512 * 4608, 49, 4608, 512)
    assert f["head"] == 2.0 * 512 * 1000
    assert f["frame"] == f["stem"] + sum(c[1] for c in f["convs"]) + f["head"]
    assert 3.6e9 < f["frame"] < 3.7e9                                           # ResNet-18: 1.8 GMAC
    assert f["workspace_floats"] == 56 * 56 * 64 * 5 + 28 * 28 * 128 * 5 + 14 * 14 * 256 * 5 + 7 * 7 * 512 * 5 + 512
    # an odd shape: 34 x 70 -> conv 17 x 35 -> pooled 9 x 18 -> 5 x 9 -> 3 x 5 -> 2 x 3
    assert RP.resnet_maps(34, 70) == [(9, 18), (9, 18), (5, 9), (3, 5), (2, 3)]
    g = RP.resnet_flops(34, 70, 7)
    assert g["stem"] == 2.0 * 17 * 35 * 64 * 147 and g["head"] == 2.0 * 512 * 7
    gc = {n: fl for n, fl, *_ in g["convs"]}
    assert gc["out1"] == 2.0 * 9 * 18 * 64 * 576 and gc["down4"] == 2.0 * 3 * 5 * 256 * 128 and gc["mid6"] == 2.0 * 2 * 3 * 512 * 2304


def test_binding_exports_the_plan():
    names = [f"rva_resnet_plan_{n}" for n in ("create", "destroy", "info", "run", "run_post", "stage")]
    assert all(n in N.EXPORTS for n in names) and "rva_resnet.hip" in N.SOURCES
    assert RP.ENGINE == "resnet-f32" and RP.FusedResNet18.ABI == "rva_resnet_plan"
    L = N.lib()
    assert all(hasattr(L, n) for n in names)
    assert [f[0] for f in N.ResNetDesc._fields_] == ["height", "width", "classes", "top_k", "max_frames"]
