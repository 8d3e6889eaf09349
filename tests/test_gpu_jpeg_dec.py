"""K8 on the GPU: the device JPEG decoder's BGR output against Pillow's libjpeg-turbo with no tolerance, its NV12 output against
the formulas of include/rva.h applied to the planes of tests/jpeg_ref.py (whose RGB tests/test_jpeg_dec_host.py pins to Pillow),
batches against single calls, failure isolation, and Motion-JPEG streams through to track tables."""
import asyncio
import copy

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd import video_stream as V
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
from tests import jpeg_ref as J

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL.Image")


def _bgr(data):
    return J.pillow_rgb(data)[..., ::-1]


def _same(t, want):
    return t is not None and np.array_equal(t.cpu().numpy(), want)


@pytest.fixture(scope="module")
def dec():
    d = ops.JpegBatchDecoder(64, (128, 96), 1 << 16)
    yield d
    d.close()


@pytest.mark.parametrize("size", J.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bgr_equals_pillow_on_the_grid(dec, size):
    """Sizes x sampling x quality 5 / 50 / 90 / 100 x restart none / 1 / 3 MCUs: 36 streams per size, one batch, every picture
    bit-identical to Pillow's."""
    cases = [(name, data) for name, data in J.grid() if name.startswith(f"{size[0]}x{size[1]}-")]
    assert len(cases) == 36
    got = dec.decode([d for _, d in cases], "bgr")
    assert dec.status == [0] * 36
    for (name, data), t in zip(cases, got):
        assert tuple(t.shape) == (size[1], size[0], 3) and _same(t, _bgr(data)), name


def test_bgr_grayscale_optimized_huffman_custom_qtables_and_small_widths():
    gray = J.encode(J.make_image(19, 21, 3)[..., 0], 90)
    img = J.make_image(33, 47, 5)
    cases = {"gray": gray, "optimize": J.encode(img, 75, 2, optimize=True), "optimize-444-r": J.encode(img, 30, 0, optimize=True, restart_marker_blocks=2),
             "qtables": J.encode(img, 90, 1, qtables=[list(range(1, 65)), [7] * 64]),
             "3x5": J.encode(J.make_image(3, 5, 1), 90, 1), "4x9": J.encode(J.make_image(4, 9, 1), 90, 2), "rows": J.encode(img, 60, 2, restart_marker_rows=1)}
    for name, data in cases.items():
        assert _same(ops.jpeg_decode_bgr(data), _bgr(data)), name
    with pytest.raises(ValueError, match="SOF2"):
        ops.jpeg_decode_bgr(J.encode(img, 90, 2, progressive=True))


def test_k7_round_trip():
    """K7's own streams (4:2:0, one restart interval per MCU row) decode to what Pillow decodes from the same bytes."""
    for (w, h) in [(48, 40), (100, 75)]:
        img = torch.from_numpy(np.ascontiguousarray(J.make_image(w, h, w)[..., ::-1])).cuda()
        for q in (30, 95):
            data = ops.jpeg_encode_bgr(img, q)
            assert ops.jpeg_probe(data)["intervals"] == -(-h // 16)
            assert _same(ops.jpeg_decode_bgr(data), _bgr(data)), (w, h, q)


def _mixed8():
    spec = [(17, 13, 0, 0), (40, 48, 2, 1), (33, 47, 1, 3), (16, 16, 2, 0), (100, 75, 2, 2), (15, 34, 0, 5), (8, 8, 1, 0), (64, 48, 2, 4)]
    out = [J.encode(J.make_image(w, h, 50 + i), 80, sub, **({"restart_marker_blocks": r} if r else {})) for i, (w, h, sub, r) in enumerate(spec)]
    out[3] = J.encode(J.make_image(19, 21, 3)[..., 0], 70)
    return out


def test_batch_of_mixed_images_equals_single_calls_on_two_streams():
    datas = _mixed8()
    singles = [ops.jpeg_decode_bgr(d).cpu().numpy() for d in datas]
    for s, d in zip(singles, datas):
        assert np.array_equal(s, _bgr(d))
    a, b = ops.JpegBatchDecoder(8, (128, 96), 1 << 16), ops.JpegBatchDecoder(8, (128, 96), 1 << 16)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        ra = a.decode(datas, "bgr")
    with torch.cuda.stream(sb):
        rb = b.decode(datas[::-1], "bgr")
    torch.cuda.synchronize()
    assert a.status == [0] * 8 and b.status == [0] * 8
    for i in range(8):
        assert _same(ra[i], singles[i]) and _same(rb[7 - i], singles[i]), i
    a.close(); b.close()


def test_limits_and_argument_errors(dec):
    small = ops.JpegBatchDecoder(2, (32, 32), 1024)
    ok, wide = J.encode(J.make_image(16, 16, 1), 90, 2), J.encode(J.make_image(40, 16, 1), 90, 2)
    got = small.decode([wide, ok], "bgr")
    assert got[0] is None and "40x16" in small.errors[0] and "32x32" in small.errors[0] and small.status[0] == N.RVA_JPEG_DEC_REFUSED
    assert _same(got[1], _bgr(ok))
    big = J.encode(J.make_image(32, 32, 1), 100, 0)
    assert len(big) > 1024 + 700
    got = small.decode([ok, big], "bgr")
    assert got[1] is None and small.status == [0, N.RVA_JPEG_DEC_REFUSED] and _same(got[0], _bgr(ok))
    with pytest.raises(RuntimeError, match="3 images, the decoder was created for 1..2"):
        small.decode([ok, ok, ok], "bgr")
    with pytest.raises(RuntimeError, match="even sizes only"):
        small.decode([J.encode(J.make_image(17, 13, 1), 90, 2)], "nv12")
    small.close()


def _scan_start(data):
    p = 2
    while True:
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        p += 2 + n
        if m == 0xDA:
            return p


def test_failure_isolation(dec):
    """A damaged picture reports a failure (or, for flips that stay decodable, a success); its neighbours are bit-identical to
    their single decodes."""
    datas = [J.encode(J.make_image(40, 48, 20 + i), 85, sub, **kw) for i, (sub, kw) in
             enumerate([(2, {}), (1, {"restart_marker_blocks": 2}), (0, {}), (2, {"restart_marker_rows": 1})])]
    want = [_bgr(d) for d in datas]
    # image 2 truncated in its scan
    cut = list(datas)
    cut[2] = datas[2][:_scan_start(datas[2]) + (len(datas[2]) - _scan_start(datas[2])) // 2]
    got = dec.decode(cut, "bgr")
    assert dec.status[2] in (N.RVA_JPEG_DEC_FAILED, N.RVA_JPEG_DEC_REFUSED) and got[2] is None
    assert [dec.status[i] for i in (0, 1, 3)] == [0, 0, 0] and all(_same(got[i], want[i]) for i in (0, 1, 3))
    # the same with no DRI in the damaged picture's neighbours swapped: image 1 (with restart markers) cut
    cut = list(datas)
    cut[1] = datas[1][:_scan_start(datas[1]) + 200]
    got = dec.decode(cut, "bgr")
    assert dec.status[1] < 0 and got[1] is None and all(_same(got[i], want[i]) for i in (0, 2, 3))
    # image 1: 16 seeded byte flips in its scan
    rng = np.random.default_rng(5)
    b = bytearray(datas[1])
    s0 = _scan_start(datas[1])
    for p in rng.integers(s0, len(b) - 2, 16):
        b[int(p)] ^= int(rng.integers(1, 256))
    flipped = list(datas)
    flipped[1] = bytes(b)
    got = dec.decode(flipped, "bgr")
    assert dec.status[1] in (0, N.RVA_JPEG_DEC_FAILED, N.RVA_JPEG_DEC_REFUSED) and (got[1] is None) == (dec.status[1] != 0)
    assert [dec.status[i] for i in (0, 2, 3)] == [0, 0, 0] and all(_same(got[i], want[i]) for i in (0, 2, 3))
    # and the object is as good as new
    got = dec.decode(datas, "bgr")
    assert dec.status == [0] * 4 and all(_same(got[i], want[i]) for i in range(4))


@pytest.mark.parametrize("size", [(16, 16), (34, 18), (48, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nv12_equals_the_formulas_on_the_helper_planes(dec, size):
    w, h = size
    pitch = 64
    datas = [J.encode(J.make_image(w, h, 9), 85, sub, **kw) for sub, kw in [(2, {}), (1, {"restart_marker_blocks": 2}), (0, {}), (2, {"restart_marker_rows": 1})]]
    datas.append(J.encode(J.make_image(w, h, 9, ramp=True)[..., 1], 85))
    outs = [ops.Nv12Surface(torch.full((h, pitch), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((h // 2, pitch), 0xCD, dtype=torch.uint8, device="cuda"), w, h)
            for _ in datas]
    got = dec.decode(datas, "nv12", out=outs)
    assert dec.status == [0] * len(datas)
    for i, data in enumerate(datas):
        ref = J.decode(data)
        assert np.array_equal(ref["rgb"], J.pillow_rgb(data))
        y, uv = J.nv12_expected(ref)
        gy, guv = got[i].y.cpu().numpy(), got[i].uv.cpu().numpy()
        assert got[i] is outs[i] and np.array_equal(gy[:, :w], y) and np.array_equal(guv[:, :w], uv), i
        assert (gy[:, w:] == 0xAB).all() and (guv[:, w:] == 0xCD).all(), "bytes beyond the width were written"
        assert 16 <= gy[:, :w].min() and gy[:, :w].max() <= 235 and 16 <= guv[:, :w].min() and guv[:, :w].max() <= 240
    alloc = dec.decode(datas[:1], "nv12")[0]                                     # allocated by the call: packed
    assert alloc.pitch == w and np.array_equal(alloc.y.cpu().numpy(), J.nv12_expected(J.decode(datas[0]))[0])


# ------------------------------------------------------------------------------------------ MjpegStream
def _rect_frames(w, h, n, seed):
    """n RGB frames: a textured background with a bright rectangle that moves."""
    base = J.make_image(w, h, seed) // 3
    out = []
    for t in range(n):
        f = base.copy()
        x0, y0 = 8 + 10 * t + 3 * seed % 7, 10 + 6 * t
        f[y0:y0 + h // 3, x0:x0 + w // 4] = (250, 240, 60)
        out.append(f)
    return out


def _write_mjpeg(path, frames, quality=85, **kw):
    datas = [J.encode(f, quality, 2, **kw) for f in frames]
    path.write_bytes(b"".join(datas))
    return datas


def _surf_np(s):
    return s.y[:, :s.width].cpu().numpy(), s.uv[:, :s.width].cpu().numpy()


def _expected_nv12(data):
    return J.nv12_expected(J.decode(data))


def _eq_surface(surf, want):
    y, uv = _surf_np(surf)
    return np.array_equal(y, want[0]) and np.array_equal(uv, want[1])


def test_mjpeg_stream_frames_end_hold_and_reopen(tmp_path):
    datas = _write_mjpeg(tmp_path / "cam.mjpeg", _rect_frames(64, 48, 5, 1), restart_marker_rows=1)
    want = [_expected_nv12(d) for d in datas]
    cfg = StreamConfig(name="cam", url=f"file://{tmp_path / 'cam.mjpeg'}", warmup_seconds=0.0, reconnect_backoff=0.5)
    s = V.open_stream(cfg)
    assert isinstance(s, V.MjpegStream) and s.hold == 4
    pkts = [s.next_packet() for _ in range(5)]
    assert [p.frame_id for p in pkts] == [0, 1, 2, 3, 4] and s.info["frames"] == 5 and s.info["width"] == 64
    assert all(_eq_surface(p.frame, w) for p, w in zip(pkts, want))              # frame 0 is still intact after hold = 4 more frames
    assert s.next_packet() is None and s.next_surface() is None                  # the end of the file is a failed read
    s.close_sync()
    # the inherited capture loop: three failed reads, a reopen, frames from 0 again
    sleeps = []

    async def run():
        async def fake_sleep(t):
            sleeps.append(t)
        s._sleep = fake_sleep
        seen = []
        async for p in s.frames():
            seen.append((p.frame_id, _eq_surface(p.frame, want[p.frame_id])))
            if len(seen) == 8:
                break
        return seen
    seen = asyncio.run(run())
    assert seen == [(i, True) for i in (0, 1, 2, 3, 4, 0, 1, 2)]
    assert sleeps == [0.5 * 1.5, 0.5 * 2.0, 0.5 * 2.5]                           # back-off of the three misses before the reopen
    # a still is a one-frame stream
    (tmp_path / "one.jpg").write_bytes(datas[2])
    one = V.open_stream(StreamConfig(name="still", url=str(tmp_path / "one.jpg"), warmup_seconds=0.0))
    assert _eq_surface(one.next_packet().frame, want[2]) and one.next_packet() is None


def test_mjpeg_hold_recycles_after_hold_frames(tmp_path):
    datas = _write_mjpeg(tmp_path / "cam.mjpg", _rect_frames(64, 48, 5, 2))
    s = V.MjpegStream(StreamConfig(name="cam", url=str(tmp_path / "cam.mjpg"), warmup_seconds=0.0), hold=2)
    first = s.next_packet().frame
    want0 = _expected_nv12(datas[0])
    s.next_packet(); s.next_packet()
    assert _eq_surface(first, want0)                                             # valid for hold = 2 further frames
    third = s.next_packet().frame
    assert third is first and _eq_surface(third, _expected_nv12(datas[3]))       # then the ring comes round


def test_next_packets_equals_per_stream_next_packet(tmp_path):
    files = []
    for i, (w, h) in enumerate([(64, 48), (128, 96), (32, 32)]):
        _write_mjpeg(tmp_path / f"c{i}.mjpeg", _rect_frames(w, h, 2 + i, 3 + i), **({"restart_marker_blocks": 3} if i else {}))
        files.append(str(tmp_path / f"c{i}.mjpeg"))
    mk = lambda: [V.MjpegStream(StreamConfig(name=f"c{i}", url=f, warmup_seconds=0.0)) for i, f in enumerate(files)]
    a, b = mk(), mk()
    for t in range(5):
        together = V.MjpegStream.next_packets(a)
        alone = [s.next_packet() for s in b]
        assert [p is None for p in together] == [p is None for p in alone] == [t >= 2 + i for i in range(3)]
        for p, q in zip(together, alone):
            if p is not None:
                assert p.frame_id == q.frame_id == t and p.stream.name == q.stream.name
                assert all(np.array_equal(x, y) for x, y in zip(_surf_np(p.frame), _surf_np(q.frame)))


class _ListSource(V._BaseStream):
    def __init__(self, cfg, surfaces):
        super().__init__(cfg)
        self.surfaces = surfaces

    def next_surface(self):
        return self.surfaces[self._frame_id] if self._frame_id < len(self.surfaces) else None


def test_end_to_end_mjpeg_to_tracks(tmp_path, monkeypatch):
    """bytes in a file -> frames in HBM -> K1 -> YOLOv8n plan -> tracks, against the same pipeline fed the expected NV12 planes."""
    from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
    from realtime_video_analytics_32streams_amd.engine import FusedYoloV8
    from realtime_video_analytics_32streams_amd.pipeline import TickPipeline
    from realtime_video_analytics_32streams_amd.tracker import IouTracker
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density
    monkeypatch.setattr(FusedYoloV8, "autotune", lambda self, reps=5: None)      # autotune=False: the default kernel selection
    streams = [StreamConfig(name=f"cam{i}", url=str(tmp_path / f"cam{i}.mjpeg"), warmup_seconds=0.0) for i in range(2)]
    datas = [_write_mjpeg(tmp_path / f"cam{i}.mjpeg", _rect_frames(128, 96, 3, 4 + i), restart_marker_rows=1) for i in range(2)]
    expect = [[ops.Nv12Surface.from_numpy(*_expected_nv12(d), 128, 96) for d in ds] for ds in datas]
    dcfg = DetectorConfig(model_path="yolov8n.pt", backend="hip", model_type="yolov8", warmup=False, half=True, confidence_threshold=0.25)
    net = HipYoloDetector(dcfg, net=build_detector_net("n", seed=0)).net       # on the device, in the plan's precision
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([e[0] for e in expect], (640, 640), half=True)
    calibrate_detection_density(net, sample.contiguous(memory_format=torch.channels_last), 0.25, 20)
    tcfg = TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1)

    def run(sources):
        det = HipYoloDetector(dcfg, net=copy.deepcopy(net))
        pipe = TickPipeline(streams, det, IouTracker(tcfg, max_streams=2), sources=sources)
        return [{k: [(t.track_id, t.class_id, t.age, t.hits, t.confidence, t.bbox_xyxy) for t in v] for k, v in pipe.tick().tracks.items()}
                for _ in range(3)]
    got = run([V.open_stream(s) for s in streams])
    want = run([_ListSource(s, e) for s, e in zip(streams, expect)])
    assert got == want
    assert sum(len(v) for tick in got for v in tick.values()) > 0, "the calibrated detector produced no tracks"
