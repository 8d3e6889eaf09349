"""A detector trained on its own class list: the module, and ``build_detector_net`` reading the class count from a checkpoint
(CPU).  The GPU side of the feature is tests/test_gpu_head_nc.py (the three ``_nc`` head entries) and tests/test_gpu_plan_nc.py
(the plans, the detector and the pipeline)."""
import pytest
import torch

from realtime_video_analytics_32streams_amd import yolov8 as Y


@pytest.mark.parametrize("nc", [1, 3, 91])
def test_module_returns_four_plus_nc_rows(nc):
    """64 x 96: 8 x 12 + 4 x 6 + 2 x 3 = 126 anchors.  91: the class branch's interior width follows the class count (91 > 64)."""
    net = Y.YoloV8("n", nc).eval()
    with torch.inference_mode():
        out = net(torch.zeros((1, 3, 64, 96)))
    assert tuple(out.shape) == (1, 4 + nc, 126)
    assert net.detect.cls[0][2].out_channels == nc and net.detect.cls[0][1].conv.out_channels == max(64, nc)


def _ultralytics_names(sd):
    inv = {v: k for k, v in Y._ULTRALYTICS_LAYERS.items()}
    theirs = {}
    for k, v in sd.items():
        head, _, rest = k.partition(".")
        if head == "detect":
            branch, _, tail = rest.partition(".")
            theirs[f"model.22.{'cv2' if branch == 'box' else 'cv3'}.{tail}"] = v
        else:
            theirs[f"model.{inv[head]}.{rest}"] = v
    theirs["model.22.dfl.conv.weight"] = torch.arange(16.0).view(1, 16, 1, 1)
    return theirs


@pytest.mark.parametrize("naming", ["own", "ultralytics"])
def test_class_count_comes_from_the_checkpoint(tmp_path, naming):
    torch.manual_seed(3)
    src = Y.YoloV8("n", 3)
    sd = src.state_dict() if naming == "own" else _ultralytics_names(src.state_dict())
    assert Y.checkpoint_class_count(sd) == 3
    f = tmp_path / "yolov8n-three.pt"
    torch.save(sd, f)
    net = Y.build_detector_net("n", weights=str(f))
    assert net.nc == 3 and not net.training
    a, b = src.state_dict(), net.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert Y.build_detector_net("n", weights=str(f), nc=3).nc == 3          # an explicit count the file agrees with
    with pytest.raises((RuntimeError, ValueError), match="shape|size mismatch"):
        Y.build_detector_net("n", weights=str(f), nc=80)                    # ... and one it contradicts: the loader's shape error


def test_no_checkpoint_gives_eighty_classes(tmp_path):
    assert Y.build_detector_net("n").nc == 80
    assert Y.build_detector_net("n", weights=str(tmp_path / "absent.pt")).nc == 80      # a name that is no file: seeded weights
    assert Y.build_detector_net("n", nc=20).nc == 20
    assert Y.checkpoint_class_count({"b0.conv.weight": torch.zeros(1)}) is None


def test_density_shifts_of_a_one_class_head():
    """A 5-row head is plain scores (no objectness column): one shift, bisected to the target count."""
    z = torch.linspace(-8.0, 2.0, 4 * 500).view(4, 1, 500)
    s0, sr = Y.density_shifts(z, 0.25, 50)
    assert sr == 0.0
    n = int((torch.sigmoid(z[:, 0] + s0) >= 0.25).sum())
    assert abs(n - 200) <= 2
