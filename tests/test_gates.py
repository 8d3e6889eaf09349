"""Frame gates.  CPU: adaptive-fps schedule against the reference's StreamWorker recording.
GPU: K5 motion gate against the oracle restatement; gated ticks in the pipeline."""
import numpy as np
import pytest

from realtime_video_analytics_32streams_amd.config import StreamConfig
from realtime_video_analytics_32streams_amd.gates import AdaptiveFps
from tests.conftest import load_golden


def test_adaptive_fps_schedule_matches_reference_worker():
    for case in load_golden("adaptive_fps.json"):
        st = StreamConfig(name="s", url="x", adaptive_fps=True, **case["cfg"])
        g = AdaptiveFps(st)
        processed, updates = [], []
        for f, n_det in enumerate(case["script"]):
            if g.should_process():
                processed.append(f)
                updates.append(n_det)
                g.update(n_det, n_det)          # the golden's stand-in tracker returns its detections as tracks
            else:
                updates.append(0)
                g.update(0, 0)
        assert processed == case["processed"]
        assert updates == case["tracker_updates"]


_FIXED_THRESHOLDS = [0.0, 1.0, 1.5, -0.1, 0.02, 0.3, 0.9, 1e-9, 0.999999, 0.5, 1.0 / 3.0, 0.01, 0.001]


def test_motion_min_count_is_the_reference_float_compare():
    """gates.motion_min_count (what the device gate in K4 compares the K5 count with) against the reference's decision
    ``changed / float(total) >= threshold`` by brute force: for every n in 1..199 and every threshold that can sit on a
    decision boundary -- each quotient c/n itself and its two float neighbours -- plus the fixed set, the result is the
    smallest c in [0, n] whose quotient passes, or n + 1 when none does (threshold above 1)."""
    from realtime_video_analytics_32streams_amd.gates import motion_min_count
    cases = 0
    for n in range(1, 200):
        q = np.arange(n + 1, dtype=np.float64) / float(n)            # IEEE double division, as float(c) / float(n)
        thr = np.concatenate([q, np.nextafter(q, np.inf), np.nextafter(q, -np.inf), _FIXED_THRESHOLDS])
        ok = q[None, :] >= thr[:, None]
        want = np.where(ok.any(1), ok.argmax(1), n + 1)
        got = [motion_min_count(float(t), n) for t in thr]
        assert got == want.tolist(), (n, [(float(t), g, int(x)) for t, g, x in zip(thr, got, want) if g != x][:5])
        cases += len(thr)
    assert cases == 3 * (199 * 200 // 2 + 199) + 199 * len(_FIXED_THRESHOLDS)


@pytest.mark.parametrize("n", [640 * 360, 1920 * 1080])
def test_motion_min_count_at_frame_sizes(n):
    """At real frame sizes brute force is too long; the two inequalities that define the result are checked instead:
    c passes (or is n + 1: nothing passes) and c - 1 does not (or c is 0)."""
    from realtime_video_analytics_32streams_amd.gates import motion_min_count
    cs = np.array([0, 1, 2, n // 100, n // 50, n // 3, n // 2, n - 1, n, 12345, 4608, 6221], dtype=np.float64)
    q = cs / float(n)
    for t in np.concatenate([q, np.nextafter(q, np.inf), np.nextafter(q, -np.inf), _FIXED_THRESHOLDS]).tolist():
        c = motion_min_count(t, n)
        assert 0 <= c <= n + 1
        assert c == n + 1 or float(c) / float(n) >= t, (t, c)
        assert c == 0 or not (float(c - 1) / float(n) >= t), (t, c)


@pytest.mark.gpu
def test_motion_gate_matches_oracle_over_ticks():
    import torch
    from oracle import oracle as orc
    from realtime_video_analytics_32streams_amd import ops, synth
    from realtime_video_analytics_32streams_amd.gates import MotionGate
    w, h, S, T = 640, 360, 3, 5
    thr = [0.02, 0.3, 0.9]
    gate = MotionGate(S, w, h, thr)
    prev = [None] * S
    for t in range(T):
        frames = [synth.make_nv12(100 + s, w, h, 768, tick=t * (s + 1)) for s in range(S)]
        surf = [ops.Nv12Surface.from_numpy(y, uv, w, h) for y, uv in frames]
        if t == 2:
            surf[1] = None                      # stream 1 delivers no frame this tick: its history is untouched
        got = gate.step(surf)
        for s in range(S):
            if surf[s] is None:
                assert got[s] is True
                continue
            cnt, blur = orc.motion_step_nv12(frames[s][0], frames[s][1], w, h, prev[s])
            want = True if prev[s] is None else (cnt / float(w * h)) >= thr[s]
            assert got[s] == want, (t, s, cnt)
            flip = gate._flip[s] ^ 1            # buffer just written
            assert np.array_equal(gate._blur[s][flip].cpu().numpy(), blur), (t, s)
            prev[s] = blur


@pytest.mark.gpu
def test_pipeline_applies_motion_and_adaptive_gates():
    import torch
    from realtime_video_analytics_32streams_amd.config import DetectorConfig, TrackerConfig
    from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
    from realtime_video_analytics_32streams_amd.pipeline import TickPipeline
    from realtime_video_analytics_32streams_amd.tracker import IouTracker
    from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream
    streams = [StreamConfig(name="still", url="synthetic://640x360", warmup_seconds=0.0, motion_filter=True, motion_threshold=0.01),
               StreamConfig(name="moving", url="synthetic://640x360", warmup_seconds=0.0, motion_filter=True, motion_threshold=0.01),
               StreamConfig(name="idle", url="synthetic://640x360", warmup_seconds=0.0, adaptive_fps=True, target_fps=30.0,
                            min_target_fps=10.0, idle_frame_tolerance=2)]
    det = HipYoloDetector(DetectorConfig(model_path="yolov8n.pt", backend="hip", half=True, confidence_threshold=0.25, warmup=False))
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=3)
    srcs = [SyntheticNv12Stream(streams[0], index=0, width=640, height=360, n_unique=1),     # same frame every tick
            SyntheticNv12Stream(streams[1], index=1, width=640, height=360, n_unique=4),     # moving rectangles
            SyntheticNv12Stream(streams[2], index=2, width=640, height=360, n_unique=2)]
    pipe = TickPipeline(streams, det, trk, sources=srcs)
    seen = {s.name: [] for s in streams}
    calls = []
    orig = det.predict_batch_device
    det.predict_batch_device = lambda pk: (calls.append([p.stream.name for p in pk]), orig(pk))[1]
    for _ in range(8):
        pipe.tick()
    per_stream = {n: sum(n in c for c in calls) for n in seen}
    assert per_stream["still"] == 1                 # first frame processed, identical frames gated out afterwards
    assert per_stream["moving"] >= 6                # synthetic rectangles move every tick (> 1 % of the pixels)
    # random-weight detector finds nothing -> the idle stream drops to every 3rd frame after 2 idle frames
    assert 1 <= per_stream["idle"] < 8 and pipe.adaptive[2].process_every == 3


def test_rasterize_polygons_rectangles_are_inclusive():
    from realtime_video_analytics_32streams_amd.gates import rasterize_polygons
    m = rasterize_polygons([[(2, 1), (7, 1), (7, 4), (2, 4)], [(0, 0), (1, 0), (1, 1), (0, 1)]], 10, 6)
    want = np.zeros((6, 10), np.uint8); want[1:5, 2:8] = 255; want[0:2, 0:2] = 255
    assert np.array_equal(m, want)
    assert rasterize_polygons([], 4, 3).sum() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("wh", [(1920, 1080), (1000, 700)], ids=["ratio-path", "generic-path"])
def test_preprocess_with_roi_mask_matches_oracle(wh):
    import torch
    from oracle import oracle as orc
    from realtime_video_analytics_32streams_amd import ops, synth
    from realtime_video_analytics_32streams_amd.gates import rasterize_polygons
    w, h = wh
    y, uv = synth.make_nv12(11, w, h, ((w + 255) // 256) * 256)
    mask = rasterize_polygons([[(w // 8, h // 6), (w * 3 // 4, h // 5), (w * 2 // 3, h * 5 // 6), (w // 5, h * 3 // 4)]], w, h)
    s_m = ops.Nv12Surface.from_numpy(y, uv, w, h); s_m.mask = torch.from_numpy(mask).cuda()
    s_0 = ops.Nv12Surface.from_numpy(y, uv, w, h)
    out, meta = ops.preprocess_nv12([s_m, s_0], (640, 640), half=True)
    bgr = orc.nv12_to_bgr(y, uv, w, h)
    masked = bgr & (mask[..., None] // 255 * 255)            # cv2.bitwise_and(frame, frame, mask=mask)
    want_m, _ = orc.preprocess_bgr(masked, 640, 640, True)
    want_0, _ = orc.preprocess_bgr(bgr, 640, 640, True)
    got = out.cpu().numpy()
    assert np.array_equal(got[0].view(np.uint16), want_m.view(np.uint16))
    assert np.array_equal(got[1].view(np.uint16), want_0.view(np.uint16))      # an unmasked stream in the same launch


@pytest.mark.gpu
def test_downsample_stage_and_box_rescale_match_oracle():
    import torch
    from oracle import oracle as orc
    from realtime_video_analytics_32streams_amd import _native as N, ops, synth
    w, h, ratio = 1920, 1080, 0.6
    dw, dh = int(w * ratio), int(h * ratio)
    y, uv = synth.make_nv12(12, w, h, 2048)
    surf = ops.Nv12Surface.from_numpy(y, uv, w, h)
    small = ops.resize_nv12_to_bgr([surf], (dw, dh))
    want_small = orc.resize_linear(orc.nv12_to_bgr(y, uv, w, h), dw, dh)       # downsample(): cv2.resize INTER_LINEAR
    assert np.array_equal(small[0].cpu().numpy(), want_small)
    out, meta = ops.preprocess_bgr([small[0]], (640, 640), half=True)
    want, m = orc.preprocess_bgr(want_small, 640, 640, True)
    assert meta.as_meta() == m and np.array_equal(out.cpu().numpy()[0].view(np.uint16), want.view(np.uint16))
    # _rescale_detections: float64 multiply by 1/max(ratio,1e-6) on the way into the tracker
    scale = 1.0 / max(ratio, 1e-6)
    head = np.ascontiguousarray(synth.make_head(3, n_obj=10).T)
    post = ops.postprocess(torch.from_numpy(head).cuda()[None], 0.25, 0.45, None, [N.letterbox(dw, dh, 640, 640)])
    trk = ops.DeviceTracker(1, 30, 0.5, 1, capacity=128)
    trk.set_box_scale([scale])
    trk.update_from_post([0], post, 0.25)
    trk.assign_ids()
    tab = trk.read(0)
    ref = orc.postprocess(head, 0.25, 0.45, None, (dw, dh))
    ref_boxes = ref["boxes"].astype(np.float64) * scale
    otr = orc.Tracker(1, 30, 0.5, 1)
    keep = ref["conf"].astype(np.float64) >= 0.25
    wtab = otr.update(0, ref_boxes[keep], ref["conf"].astype(np.float64)[keep], ref["cls"].astype(np.int64)[keep])
    assert orc.table_of(tab) == orc.table_of(wtab)


@pytest.mark.gpu
def test_pipeline_with_roi_and_downsample_runs_reference_order():
    import torch
    from oracle import oracle as orc
    from realtime_video_analytics_32streams_amd import ops
    from realtime_video_analytics_32streams_amd.config import DetectorConfig, TrackerConfig
    from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
    from realtime_video_analytics_32streams_amd.pipeline import TickPipeline
    from realtime_video_analytics_32streams_amd.tracker import IouTracker
    from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream
    roi = [[(100, 50), (1700, 80), (1600, 1000), (200, 900)]]
    streams = [StreamConfig(name=f"cam{i}", url="synthetic://1920x1080", warmup_seconds=0.0, downsample_ratio=0.5,
                            roi_polygons=roi if i == 0 else None, motion_filter=(i == 1), motion_threshold=0.0) for i in range(2)]
    seen = {}
    det = HipYoloDetector(DetectorConfig(model_path="yolov8n.pt", backend="hip", half=True, confidence_threshold=0.25, warmup=False))
    orig = det._preprocess
    det._preprocess = lambda frames: (seen.setdefault("frames", frames), orig(frames))[1]
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=2)
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=2) for i, s in enumerate(streams)]
    pipe = TickPipeline(streams, det, trk, sources=srcs)
    pipe.tick()
    frames = seen["frames"]
    assert all(isinstance(f, torch.Tensor) and tuple(f.shape) == (540, 960, 3) for f in frames)   # downsampled BGR reached the detector
    s0 = srcs[0]._ring[0]
    bgr = orc.nv12_to_bgr(s0.y.cpu().numpy(), s0.uv.cpu().numpy(), 1920, 1080)
    mask = pipe._roi_masks[0].cpu().numpy()
    want = orc.resize_linear(bgr & (mask[..., None] // 255 * 255), 960, 540)
    assert np.array_equal(frames[0].cpu().numpy(), want)                                           # roi -> downsample order
    assert trk.device_tracker.state()[1] == 0
