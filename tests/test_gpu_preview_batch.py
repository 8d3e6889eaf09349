"""Batched previews on the device: K7 as an encoder object that owns its scratch (``rva_jpeg_batch_*`` /
``ops.JpegBatchEncoder``), K6 for a whole tick in one launch (``rva_preview_nv12_batch``), ``preview.render_frames`` and the
``TickPipeline.previews`` hook.  Every JPEG stream is held to ``oracle/jpeg_oracle.py`` byte for byte, every K6 image to the
single-surface kernel, every data URL to ``preview.render_frame``."""
import base64
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import jpeg_oracle as J
from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops, synth, wire
from realtime_video_analytics_32streams_amd import preview as P

pytestmark = pytest.mark.gpu

MIXED = [(72, 40, 80), (8, 8, 30), (1, 1, 75), (17, 9, 100), (250, 123, 50), (333, 201, 90), (96, 64, 60), (640, 360, 75)]


@functools.lru_cache(maxsize=None)
def _case(w, h, q):
    """(host image, the oracle's stream) of one standard case: computed once, shared by every test, never modified."""
    bgr = synth.make_bgr(31 + w + q, w, h)
    bgr.setflags(write=False)
    return bgr, J.encode(bgr, q)


def _dev(cases):
    return [torch.from_numpy(_case(*c)[0]).cuda() for c in cases]


def _want(cases):
    return [_case(*c)[1] for c in cases]


def _qs(cases):
    return [c[2] for c in cases]


@pytest.fixture(scope="module")
def enc():
    e = ops.JpegBatchEncoder(8, (640, 360))
    yield e
    e.close()


def test_mixed_batch_is_the_oracles_bytes(enc):
    """Eight sizes and eight qualities in ONE launch set: one block, one interval, odd edges with dummy luma blocks, 2 and 4
    entropy passes per interval (250 / 333 / 640 wide), 23 intervals, eight different quantisation tables."""
    syncs = enc.host_syncs
    got = enc.encode(_dev(MIXED), _qs(MIXED))
    assert enc.host_syncs - syncs == 2, "two host synchronisations per batch, whatever n"
    for c, g, w in zip(MIXED, got, _want(MIXED)):
        assert len(g) == len(w), (c, len(g), len(w))
        assert g == w, c


def test_position_independence_and_bounds(enc):
    rev = MIXED[::-1]
    assert enc.encode(_dev(rev), _qs(rev)) == _want(rev)
    c = (250, 123, 50)
    others = [m for m in MIXED if m != c]
    assert enc.encode(_dev([c]), [c[2]]) == [_case(*c)[1]]                                   # alone
    assert enc.encode(_dev([c] + others), _qs([c] + others))[0] == _case(*c)[1]              # first of 8 == max_images
    assert enc.encode(_dev(others + [c]), _qs(others + [c]))[-1] == _case(*c)[1]             # last of 8
    # outside the object's bounds: the argument error, nothing launched (the sizes buffer keeps the previous batch's values)
    before = enc._sizes.clone()
    with pytest.raises(RuntimeError, match=r"status 1.*created for 1\.\.8"):
        enc.encode(_dev(MIXED + [(8, 8, 30)]), _qs(MIXED) + [30])
    big = torch.zeros((368, 640, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=r"status 1.*640x368.*up to 640x360"):
        enc.encode([big], [75])
    torch.cuda.synchronize()
    assert torch.equal(enc._sizes, before)
    assert enc.encode(_dev([c]), [c[2]]) == [_case(*c)[1]]


def test_a_small_batch_after_a_large_one_is_clean(enc):
    assert enc.encode(_dev(MIXED), _qs(MIXED)) == _want(MIXED)
    small = [(17, 9, 100), (1, 1, 75)]
    assert enc.encode(_dev(small), _qs(small)) == _want(small)                                # no stale sizes, offsets or flags


def test_two_encoders_on_two_streams_do_not_share_scratch(enc):
    """The ADVICE scenario: two encodes in flight at once.  Each object owns its scratch, so both are the oracle's bytes."""
    other = ops.JpegBatchEncoder(4, (640, 360))
    try:
        a, b = [(640, 360, 75), (333, 201, 90), (250, 123, 50)], [(96, 64, 60), (640, 360, 75), (72, 40, 80), (17, 9, 100)]
        ia, ib = _dev(a), _dev(b)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        cur = torch.cuda.current_stream()
        s1.wait_stream(cur); s2.wait_stream(cur)
        with torch.cuda.stream(s1):
            enc.enqueue(ia, _qs(a))
        with torch.cuda.stream(s2):                                  # no host wait between the two
            other.enqueue(ib, _qs(b))
        assert other.fetch() == _want(b)
        assert enc.fetch() == _want(a)
    finally:
        other.close()


def test_an_image_the_output_does_not_hold_reports_minus_one(enc):
    """Through the C call with a capacity that holds images 0 and 1 but not 2: sizes [ok, ok, -1], the first two streams intact
    and packed back to back; the next batch on the object is clean."""
    cases = [(250, 123, 50), (96, 64, 60), (333, 201, 90), (72, 40, 80)]
    want = _want(cases)
    cap = len(want[0]) + len(want[1]) + len(want[2]) - 1
    out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(4, dtype=torch.int32, device="cuda")
    enc.encode_into(_dev(cases[:3]), _qs(cases[:3]), out, cap, sizes)
    assert sizes.cpu().tolist()[:3] == [len(want[0]), len(want[1]), -1]
    host = out.cpu().numpy()
    assert host[:len(want[0])].tobytes() == want[0] and host[len(want[0]):len(want[0]) + len(want[1])].tobytes() == want[1]
    assert not host[len(want[0]) + len(want[1]):].any(), "the failed image takes no bytes"
    # an image after the failed one that still fits packs on behind image 1
    out.zero_()
    enc.encode_into(_dev(cases), _qs(cases), out, cap, sizes)
    assert sizes.cpu().tolist() == [len(want[0]), len(want[1]), -1, len(want[3])]
    at = len(want[0]) + len(want[1])
    assert out.cpu().numpy()[at:at + len(want[3])].tobytes() == want[3]
    assert enc.encode(_dev(cases), _qs(cases)) == want


def _tracks(n, w, h, seed=0, right_edge=False):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        bw, bh = int(rng.integers(w // 8, w // 3)), int(rng.integers(h // 8, h // 3))
        x0, y0 = float(rng.integers(0, w - bw)), float(rng.integers(0, h - bh))
        out.append({"track_id": 13 * k + 4, "class_id": int(rng.integers(0, 80)), "confidence": 0.5,
                    "bbox_xyxy": [x0 + 0.4, y0 + 0.7, x0 + bw - 0.2, y0 + bh - 0.6]})
    if right_edge and out:
        out[-1]["bbox_xyxy"][2] = float(w - 1)
    return out


def _surface(seed, w, h, pitch=None):
    y, uv = synth.make_nv12(seed, w, h, pitch)
    return ops.Nv12Surface.from_numpy(y, uv, w, h)


def _k6_single(sf, out, ratio, prims):
    rects, colors, glyphs = prims
    d = lambda a: torch.from_numpy(a).cuda() if len(a) else None     # noqa: E731
    dr, dc, dg = d(rects), d(colors), d(glyphs)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    ctx = ops.context()
    ctx.check(N.lib().rva_preview_nv12(ctx.handle, p(sf.y) if sf else None, p(sf.uv) if sf else None, sf.pitch if sf else 0,
                                       sf.width if sf else out.shape[1], sf.height if sf else out.shape[0], ratio, p(out),
                                       out.shape[1], out.shape[0], p(dr), p(dc), len(rects), p(dg), len(glyphs), 2,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rva_preview_nv12")
    torch.cuda.synchronize()
    return out


def test_batched_k6_equals_k6_per_surface():
    specs = [  # (surface, (dst w, h), ratio, tracks)
        (_surface(3, 192, 108), (192, 108), 1, _tracks(3, 192, 108, 1, right_edge=True)),
        (_surface(4, 256, 144), (128, 72), 2, _tracks(2, 128, 72, 2)),
        (_surface(5, 130, 70), (130, 70), 1, []),
        (_surface(6, 192, 108, pitch=256), (192, 108), 1, _tracks(1, 192, 108, 3)),
        (None, (100, 60), 0, _tracks(2, 100, 60, 4)),
    ]
    base = torch.from_numpy(synth.make_bgr(77, 100, 60)).cuda()
    prims = [P.raster_primitives(P.plan_render(wh, t, 75), wh) for _, wh, _, t in specs]
    assert [len(p[0]) for p in prims] == [15, 10, 0, 5, 10]
    mk = lambda wh, ratio: base.clone() if ratio == 0 else torch.full((wh[1], wh[0], 3), 7, dtype=torch.uint8, device="cuda")   # noqa: E731
    want = [_k6_single(sf, mk(wh, r), r, pr).cpu().numpy() for (sf, wh, r, _), pr in zip(specs, prims)]
    outs = [mk(wh, r) for _, wh, r, _ in specs]
    got = ops.preview_nv12_batch([s[0] for s in specs], outs, [s[2] for s in specs], prims)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.cpu().numpy(), w), k
    assert int(prims[0][0][:, 2].max()) == 191                    # the right-edge track reaches the last column
    # a persistent staging gives the same images, twice in a row
    st = ops.PreviewStaging(outs[0].device, 256)
    for _ in range(2):
        outs2 = [mk(wh, r) for _, wh, r, _ in specs]
        ops.preview_nv12_batch([s[0] for s in specs], outs2, [s[2] for s in specs], prims, staging=st)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(outs2, want))


def _decode_url(url):
    assert url.startswith("data:image/jpeg;base64,")
    return base64.b64decode(url.split(",", 1)[1])


def test_render_frames_gives_render_frames_urls():
    pol = P.PreviewPolicy(frame_quality=75)
    counts = [0, 1, 4, 11]
    surfs = [_surface(20 + i, 640, 360) for i in range(4)]
    tracks = [_tracks(n, 640, 360, 10 + n) for n in counts]
    qs = [pol.adaptive_quality(n) for n in counts]
    assert qs == [65, 75, 80, 85]
    big = _surface(30, 3840, 2160)
    big_tracks = _tracks(3, 3840, 2160, 5)
    urls = P.render_frames(surfs + [big], tracks + [big_tracks], qs + [75], pol)
    assert len(urls) == 5
    for sf, t, q, u in zip(surfs, tracks, qs, urls):
        img = P.render_nv12(sf, P.plan_render((640, 360), t, q)).cpu().numpy()
        assert _decode_url(u) == J.encode(img, q), len(t)
    assert urls[4] == P.render_frame(big, big_tracks, 75, pol)       # 4K -> 1080p (2x2 box mean) in the same batch
    assert P.render_frames([], [], [], pol) == []


def _pipeline(previews, clock_now):
    from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
    from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
    from realtime_video_analytics_32streams_amd.pipeline import TickPipeline
    from realtime_video_analytics_32streams_amd.tracker import IouTracker
    from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density
    S = 4
    streams = [StreamConfig(name=f"cam{i}", url="synthetic://640x360", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, width=640, height=360, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    if "det" not in _PIPE:
        det = HipYoloDetector(DetectorConfig(model_path="yolov8n.pt", backend="hip", model_type="yolov8", warmup=False, half=True,
                                             confidence_threshold=0.25), net=build_detector_net("n", seed=0))
        with torch.inference_mode():
            sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs], (640, 640), half=True)
        calibrate_detection_density(det.net, sample.contiguous(memory_format=torch.channels_last), 0.25, 12)
        det.invalidate_engine()
        _PIPE["det"] = det
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=S, capacity=256)
    pipe = TickPipeline(streams, _PIPE["det"], trk, sources=srcs)
    if previews:
        pipe.previews = P.PreviewBatcher(P.PreviewPolicy(frame_quality=75, clock=lambda: clock_now[0]), max_streams=S, max_wh=(640, 360))
    return pipe, srcs


_PIPE: dict = {}
CLOCK = [1000.0, 1000.05, 1000.2]            # tick 0 due, tick 1 inside the 0.1 s interval, tick 2 due again


def _tab(tracks):
    return [(t.track_id, t.class_id, t.age, t.hits, t.confidence, t.bbox_xyxy) for t in tracks]


def test_pipeline_attaches_a_ticks_previews_in_one_batch():
    now = [0.0]
    pipe, srcs = _pipeline(True, now)
    plain, _ = _pipeline(False, now)
    ref_pol = P.PreviewPolicy(frame_quality=75)
    results = []
    for k, t in enumerate(CLOCK):
        now[0] = t
        frames = [s._ring[k % 3] for s in srcs]                       # what next_packet delivers on tick k
        res = pipe.tick()
        base = plain.tick()
        assert base.frame_jpeg == {} and {n: _tab(v) for n, v in base.tracks.items()} == {n: _tab(v) for n, v in res.tracks.items()}
        if k == 1:
            assert res.frame_jpeg == {}
        else:
            assert sorted(res.frame_jpeg) == pipe.names
            for name, sf in zip(pipe.names, frames):
                tr = wire.tracks_payload(name, k, res.tracks[name])["tracks"]
                assert res.frame_jpeg[name] == P.render_frame(sf, tr, ref_pol.adaptive_quality(len(tr)), ref_pol), (k, name)
        results.append(res)
    assert sum(len(v) for v in results[0].tracks.values()) > 0, "the calibrated detector produced nothing to draw"
    _PIPE["tick_urls"] = [r.frame_jpeg for r in results]


def test_pipelined_ticks_collect_result_carries_the_same_previews():
    from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks
    if "tick_urls" not in _PIPE:
        test_pipeline_attaches_a_ticks_previews_in_one_batch()
    now = [0.0]
    pipe, _ = _pipeline(True, now)
    runner = PipelinedTicks(pipe, depth=2)
    for k, t in enumerate(CLOCK):
        now[0] = t
        runner.submit()
        res = runner.collect_result()
        assert res.tick == k and res.frame_jpeg == _PIPE["tick_urls"][k], k
