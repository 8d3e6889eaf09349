"""Host side of the YOLOv5 detector: the module (``yolov5.YoloV5``), its state-dict loaders, the architecture decision and the
engine selection of ``HipYoloDetector``, the ABI additions, and the bounds of tests/yolov5_refs.py against planted errors.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import detector as D
from realtime_video_analytics_32streams_amd import yolov5 as Y
from tests import yolov5_refs as R

# the "parameters" figure of the upstream model summaries at nc = 80 (printed for the FUSED model, see test_parameter_counts)
UPSTREAM_PARAMS = {"n": 1_867_405, "s": 7_225_885, "m": 21_172_173, "l": 46_533_693, "x": 86_705_005}


@pytest.mark.parametrize("scale", list("nsmlx"))
def test_output_shape_per_scale(scale):
    net = Y.YoloV5(scale).eval()
    with torch.inference_mode():
        assert tuple(net(torch.zeros(1, 3, 64, 64)).shape) == (1, 252, 85)


def test_25200_anchors_at_640():
    net = Y.YoloV5("n").eval()
    with torch.inference_mode():
        out = net(torch.zeros(1, 3, 640, 640))
        raw = net(torch.zeros(1, 3, 640, 640), raw=True)
    assert tuple(out.shape) == (1, 25200, 85)
    assert [tuple(r.shape) for r in raw] == [(1, 255, 80, 80), (1, 255, 40, 40), (1, 255, 20, 20)]


@pytest.mark.parametrize("scale", list("nsmlx"))
def test_parameter_counts(scale):
    """The issue quotes the upstream summaries as counts of the UNFUSED module.  They are not: the summary line upstream prints at
    detection / validation time comes after ``model.fuse()``, where every Conv-BN pair has lost the norm's weight and bias (2 c)
    and gained a convolution bias (c).  The unfused module has exactly one parameter more per BatchNorm channel (s: 7 235 389,
    the figure of upstream's training-time summary); traced to every ``ConvBnAct`` of the net, none elsewhere.  The quoted numbers
    are kept as they are and hold for the fused module."""
    net = Y.YoloV5(scale)
    unfused = sum(p.numel() for p in net.parameters())
    bn_channels = sum(m.num_features for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    fused = sum(p.numel() for p in net.fuse().parameters())
    assert fused == UPSTREAM_PARAMS[scale]
    assert unfused == UPSTREAM_PARAMS[scale] + bn_channels


def test_anchor_order():
    """Logits that encode (level, a, y, x) in the objectness entry: the output row of anchor index
    ``level offset + a*h*w + y*w + x`` carries the sigmoid of that code."""
    nc, no = 2, 7
    det = Y.Detect5(nc, (4, 4, 4)).double().eval()
    sizes = [(8, 12), (4, 6), (2, 3)]
    maps, codes = [], []
    for lv, (h, w) in enumerate(sizes):
        z = torch.zeros(1, 3 * no, h, w, dtype=torch.float64)
        a, y, x = torch.meshgrid(torch.arange(3), torch.arange(h), torch.arange(w), indexing="ij")
        code = (lv * 1000 + a * 300 + y * 20 + x).double() / 1000.0 - 1.5
        z.view(1, 3, no, h, w)[0, :, 4] = code
        maps.append(z)
        codes.append(code.reshape(-1))

    class Fixed(torch.nn.Module):
        def __init__(self, z):
            super().__init__()
            self.z = z

        def forward(self, _):
            return self.z
    det.m = torch.nn.ModuleList(Fixed(z) for z in maps)
    out = det([None, None, None])
    assert tuple(out.shape) == (1, 3 * (96 + 24 + 6), no)
    assert torch.equal(out[0, :, 4], torch.sigmoid(torch.cat(codes)))


@pytest.mark.parametrize("custom", [False, True])
def test_decode_against_a_hand_written_formula(custom):
    nc, no = 3, 8
    anchors = None if not custom else [[5, 7, 9, 11, 13, 15], [20, 30, 40, 50, 60, 70], [100, 90, 200, 210, 300, 333]]
    det = Y.Detect5(nc, (4, 4, 4), anchors).double().eval()
    table = np.array(Y.DEFAULT_ANCHORS if anchors is None else anchors, dtype=np.float64).reshape(3, 3, 2)
    rng = np.random.default_rng(3)
    sizes = [(8, 12), (4, 6), (2, 3)]
    zs = [rng.normal(0, 3, (2, 3 * no, h, w)) for h, w in sizes]

    class Fixed(torch.nn.Module):
        def __init__(self, z):
            super().__init__()
            self.z = torch.from_numpy(z)

        def forward(self, _):
            return self.z
    det.m = torch.nn.ModuleList(Fixed(z) for z in zs)
    out = det([None] * 3).numpy()
    assert out.dtype == np.float64
    base = 0
    for lv, ((h, w), z) in enumerate(zip(sizes, zs)):
        s = (8, 16, 32)[lv]
        for b in range(2):
            for a in range(3):
                for y in range(h):
                    for x in range(w):
                        sg = 1.0 / (1.0 + np.exp(-z[b, a * no:(a + 1) * no, y, x]))
                        want = sg.copy()
                        want[0] = (2 * sg[0] - 0.5 + x) * s
                        want[1] = (2 * sg[1] - 0.5 + y) * s
                        want[2] = (2 * sg[2]) ** 2 * table[lv, a, 0]
                        want[3] = (2 * sg[3]) ** 2 * table[lv, a, 1]
                        np.testing.assert_allclose(out[b, base + a * h * w + y * w + x], want, rtol=1e-13, atol=1e-13)
        base += 3 * h * w
    # the numpy restatement the GPU tests use agrees with the module
    base = 0
    for lv, ((h, w), z) in enumerate(zip(sizes, zs)):
        ref = R.head5_decode(np.ascontiguousarray(z.transpose(0, 2, 3, 1)), table[lv], (8, 16, 32)[lv], nc)
        np.testing.assert_allclose(ref.transpose(0, 2, 1), out[:, base:base + 3 * h * w], rtol=1e-13, atol=1e-13)
        base += 3 * h * w


def test_bias_initialisation():
    det = Y.Detect5(80, (8, 8, 8))
    for m, s in zip(det.m, (8, 16, 32)):
        b = m.bias.detach().view(3, 85)
        # the prior is ADDED to the default initialisation (|default| <= 1 / sqrt(8))
        assert float((b[:, 4] - np.log(8 / (640 / s) ** 2)).abs().max()) <= 8 ** -0.5 + 1e-6
        assert float((b[:, 5:] - np.log(0.6 / (80 - 0.99999))).abs().max()) <= 8 ** -0.5 + 1e-6


def _ultralytics_names(net):
    inv = {v: k for k, v in Y._ULTRALYTICS_V5_LAYERS.items()}
    out = {}
    for k, v in net.state_dict().items():
        head, _, rest = k.partition(".")
        if head == "detect":
            if rest == "anchors_px":
                out["model.24.anchors"] = v / torch.tensor([8.0, 16.0, 32.0]).view(3, 1, 1)
            else:
                out["model.24." + rest] = v
        else:
            out[f"model.{inv[head]}.{rest}"] = v
    return out


def test_state_dict_round_trip_through_ultralytics_names(tmp_path):
    anchors = [[4, 8, 12, 16, 20, 24], [32, 48, 64, 80, 96, 112], [128, 160, 192, 224, 256, 288]]     # exact in stride units
    src = Y.build_detector_net_v5("n", seed=3, nc=3, anchors=anchors)
    sd = _ultralytics_names(src)
    assert any(k.endswith("num_batches_tracked") for k in sd) and tuple(sd["model.24.anchors"].shape) == (3, 3, 2)
    assert Y.checkpoint_class_count_v5(sd) == 3 and Y.is_v5_state_dict(sd)
    f = tmp_path / "custom.pt"
    torch.save(sd, f)
    dst = Y.build_detector_net_v5("n", seed=9, weights=str(f))          # nc and anchors from the file
    assert dst.nc == 3 and torch.equal(dst.detect.anchors_px, src.detect.anchors_px)
    x = torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(1))
    with torch.inference_mode():
        assert torch.equal(src(x), dst(x))
    # the inner nn.Sequential's names (no "model." prefix) and this module's own names load too
    inner = {k[len("model."):]: v for k, v in sd.items()}
    with torch.inference_mode():
        assert torch.equal(Y.load_detector_state_dict_v5(Y.YoloV5("n", 3), inner).eval()(x), src(x))
        assert torch.equal(Y.load_detector_state_dict_v5(Y.YoloV5("n", 3), src.state_dict()).eval()(x), src(x))
    with pytest.raises(ValueError, match="does not fit YOLOv5n"):
        Y.load_detector_state_dict_v5(Y.YoloV5("n", 3), _ultralytics_names(Y.YoloV5("s", 3)))
    short = dict(sd)
    del short["model.4.cv3.conv.weight"]
    with pytest.raises(KeyError, match="lacks 1 parameters"):
        Y.load_detector_state_dict_v5(Y.YoloV5("n", 3), short)
    with pytest.raises(KeyError, match="no parameters in YOLOv5"):
        Y.load_detector_state_dict_v5(Y.YoloV5("n", 3), {**sd, "model.11.weight": torch.zeros(1)})
    assert Y.checkpoint_class_count_v5({"foo": torch.zeros(1)}) is None


def test_variant_from_path_v5():
    assert [Y.variant_from_path_v5(f"yolov5{s}.pt") for s in "nsmlx"] == list("nsmlx")
    assert Y.variant_from_path_v5("/models/YOLOv5s-custom.onnx") == "s"
    for name in ("yolov8n.pt", "yolov5.pt", "yolov5nu.pt", "yolov5su.onnx", "yolov5n6u.pt", "yolo.pt", ""):
        assert Y.variant_from_path_v5(name) is None, name


def test_architecture_decision(tmp_path):
    from realtime_video_analytics_32streams_amd.yolov8 import YoloV8
    v5_file, v5_own, v8_file = tmp_path / "weights.pt", tmp_path / "yolov8n.pt", tmp_path / "yolov5s.pt"
    torch.save(_ultralytics_names(Y.YoloV5("n", 2)), v5_file)
    torch.save(Y.YoloV5("n", 2).state_dict(), v5_own)                  # a v5 dict under a v8 NAME: the file decides
    torch.save(YoloV8("n", 2).state_dict(), v8_file)                   # a v8 dict under a v5 name: the file decides
    arch = D.detector_architecture
    assert arch("yolov8", "yolov8n.pt", net=Y.YoloV5("n", 1)) == "yolov5"
    assert arch("yolov5", "yolov5n.pt", net=YoloV8("n", 1)) == "yolov8"
    for mt in ("yolov5", "yolov8"):
        assert arch(mt, str(v5_file)) == "yolov5" and arch(mt, str(v5_own)) == "yolov5"
        assert arch(mt, str(v8_file)) == "yolov8"
    for s in "nsmlx":
        assert arch("yolov5", f"yolov5{s}.pt") == "yolov5"
        assert arch("YOLOv5", f"models/yolov5{s}-640.onnx") == "yolov5"
    # what must stay YOLOv8: the default path, every yolov8 name, the anchor-free *u re-exports, and model_type yolov8 without a file
    for mt, path in [("yolov5", "yolov8n.pt"), ("yolov5", "yolov8s.onnx"), ("yolov5", "yolov5nu.pt"), ("yolov5", "yolov5su.pt"),
                     ("yolov8", "yolov5n.pt"), ("yolov8", "yolov8n.pt"), ("yolov5", ""), ("yolov5", "best.pt")]:
        assert arch(mt, path) == "yolov8", (mt, path)
    assert D.v5_scale_of("whatever.pt", torch.load(v5_file, weights_only=True)) == "n"
    assert D.v5_scale_of("yolov5m.pt") == "m" and D.v5_scale_of("best.pt") == "n"


def test_engine_selection():
    sel = D.select_yolo_engine
    for arch in ("yolov5", "yolov8"):
        for eng in ("auto", "plan", "native"):
            assert sel(arch, True, eng) == "fused"
        assert sel(arch, False, "auto") == "torch-fp32"
    assert sel("yolov8", False, "plan") == sel("yolov8", False, "native") == "fused-f32"
    for eng in ("plan", "native"):
        with pytest.raises(ValueError, match=r"fp32 YOLOv5 plan.*half: true"):
            sel("yolov5", False, eng)


def test_abi_additions():
    new = ("rva_yolov5_plan_create", "rva_stem6_conv_f16", "rva_stem6_conv_f16_rows", "rva_conv_rows_through_pad", "rva_conv1x1_head5_f16")
    L = N.lib()
    assert all(n in N.EXPORTS and hasattr(L, n) for n in new) and L.rva_abi_version() == 1
    assert C.sizeof(N.YoloV5Desc) == 4 * (3 + 5 + 4 + 1 + 1 + 18 + 2)


def test_rows_through_the_stem():
    """Output row r of the 6x6 s2 p2 stem reads input rows 2r-2 .. 2r+3; the helper agrees with k = 1 / 3 where both exist."""
    f, g = N.lib().rva_conv_rows_through_pad, N.lib().rva_conv_rows_through
    a, b, a2, b2 = (C.c_int32() for _ in range(4))
    H = 64
    for lo in range(0, H, 5):
        for hi in range(lo + 1, H + 1, 7):
            assert f(6, 2, 2, H, lo, hi, C.byref(a), C.byref(b)) == N.RVA_OK
            want = [r for r in range(H // 2) if max(2 * r - 2, 0) < hi and min(2 * r + 4, H) > lo]
            assert (a.value, b.value) == (want[0], want[-1] + 1), (lo, hi)
            for k, s in ((1, 1), (3, 1), (3, 2)):
                assert f(k, s, k // 2, H, lo, hi, C.byref(a), C.byref(b)) == g(k, s, H, lo, hi, C.byref(a2), C.byref(b2)) == N.RVA_OK
                assert (a.value, b.value) == (a2.value, b2.value)
    assert f(6, 2, 6, H, 0, H, C.byref(a), C.byref(b)) == N.RVA_ERR_ARG and f(6, 2, 2, H, 3, 3, C.byref(a), C.byref(b)) == N.RVA_ERR_ARG


def test_density_helper():
    net = Y.build_detector_net_v5("n", seed=1, nc=3)
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(2))

    def count():
        with torch.inference_mode():
            o = net(x)
        return int(((o[..., 4] * o[..., 5:].max(-1).values) >= 0.25).sum())
    assert count() == 0                                   # a seeded head emits nothing
    Y.calibrate_detection_density_v5(net, x, 0.25, 20)
    assert 20 <= count() <= 60, count()


# ---------------------------------------------------------------------------------------- the bounds reject planted errors
def _stem_case():
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (1, 3, 32, 40)).astype(np.float16)
    w = rng.normal(0, 0.15, (16, 3, 6, 6)).astype(np.float16)
    b = rng.normal(0, 0.1, 16).astype(np.float32)
    return x, w, b


def test_stem_bound_accepts_the_restatement_and_rejects_mutants():
    x, w, b = _stem_case()
    ref, mag = R.stem6_f64(x, w, b)
    tol = R.stem6_bound(ref, mag)
    want = torch.nn.functional.silu(torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(),
                                                               torch.from_numpy(b).double(), 2, 2)).permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(ref, want, rtol=1e-12, atol=1e-12)
    assert (np.abs(R.stem6_f32_cpu(x, w, b).astype(np.float64) - ref) <= tol).all()
    for mut in R.STEM_MUTANTS:
        assert (np.abs(R.stem6_f32_cpu(x, w, b, mut=mut).astype(np.float64) - ref) > tol).any(), mut


def _head_case(nc):
    rng = np.random.default_rng(8)
    x = rng.normal(0, 1, (2, 5, 7, 64)).astype(np.float16)
    w = rng.normal(0, 0.2, (3 * (5 + nc), 64)).astype(np.float16)
    b = rng.normal(0, 0.5, 3 * (5 + nc)).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("nc", [1, 3])
def test_head_bound_accepts_the_restatement_and_rejects_mutants(nc):
    x, w, b = _head_case(nc)
    z, mag = R.logits_f64(x, w, b)
    anc, other = R.DEFAULT_ANCHORS[1], R.DEFAULT_ANCHORS[0]
    tol16, tol32, ref = R.head5_bound(z, mag, 64, anc, 16.0, nc)
    got16, got32 = R.head5_f32_cpu(x, w, b, anc, 16.0, nc)
    assert (np.abs(got16.astype(np.float64) - ref) <= tol16).all()
    assert (np.abs(got32.astype(np.float64) - ref[:, :4]) <= tol32).all()
    for mut in R.HEAD_MUTANTS:
        bad16, bad32 = R.head5_f32_cpu(x, w, b, anc, 16.0, nc, mut=mut, other_lv=other)
        assert (np.abs(bad16.astype(np.float64) - ref) > tol16).any(), mut
        assert (np.abs(bad32.astype(np.float64) - ref[:, :4]) > tol32).any(), mut
