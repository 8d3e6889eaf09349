"""K8's host half without a GPU: the marker walk behind ``ops.jpeg_probe`` (geometry, sampling, restart intervals, every refusal
by its message, a mutation corpus that must never crash), the Motion-JPEG splitter, the routing of ``open_stream``, the errors of
``MjpegStream`` that need no device, and the numpy decoder of tests/jpeg_ref.py against Pillow's libjpeg-turbo, bit for bit."""
import io

import numpy as np
import pytest

from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd import video_stream as V
from realtime_video_analytics_32streams_amd.config import StreamConfig
from tests import jpeg_ref as J

PIL = pytest.importorskip("PIL.Image")


def _good(w=16, h=16, sub=2, **kw):
    return J.encode(J.make_image(w, h, 7), 90, sub, **kw)


def _segments(data):
    """[(marker, offset of 0xFF, total bytes with the marker)] up to and including SOS."""
    out, p = [], 2
    while True:
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, 2 + n))
        p += 2 + n
        if m == 0xDA:
            return out


def _seg(data, marker, nth=0):
    return [s for s in _segments(data) if s[0] == marker][nth]


def _patch(data, off, value):
    b = bytearray(data)
    b[off] = value
    return bytes(b)


def _refused(data, match):
    with pytest.raises(ValueError, match=match):
        ops.jpeg_probe(data)


@pytest.mark.parametrize("size", J.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sampling", list(J.SAMPLINGS))
def test_probe_geometry_sampling_and_intervals(size, sampling):
    w, h = size
    hs, vs = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}[sampling]
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    img = J.make_image(w, h, 3)
    for kw, ri, n in [({}, 0, 1), ({"restart_marker_blocks": 1}, 1, mw * mh), ({"restart_marker_blocks": 3}, 3, -(-mw * mh // 3)),
                      ({"restart_marker_rows": 1}, mw, mh)]:
        info = ops.jpeg_probe(J.encode(img, 50, J.SAMPLINGS[sampling], **kw))
        assert info == dict(width=w, height=h, components=3, h_samp=hs, v_samp=vs, sampling=sampling, restart_interval=ri, intervals=n,
                            mcus=mw * mh), kw


def test_probe_grayscale_optimized_and_custom_tables():
    g = J.encode(J.make_image(19, 21, 3)[..., 0], 90)
    assert ops.jpeg_probe(g) == dict(width=19, height=21, components=1, h_samp=1, v_samp=1, sampling="gray", restart_interval=0,
                                     intervals=1, mcus=9)
    assert ops.jpeg_probe(_good(optimize=True))["sampling"] == "4:2:0"              # any DHT, not only Annex K
    assert ops.jpeg_probe(_good(qtables=[list(range(1, 65)), [7] * 64]))["width"] == 16


def test_refusals_from_pillow_streams():
    _refused(_good(progressive=True), r"SOF2 \(progressive\)")
    buf = io.BytesIO()
    PIL.fromarray(J.make_image(16, 16, 1)).convert("CMYK").save(buf, "JPEG")
    _refused(buf.getvalue(), "4 components")
    _refused(b"", "no SOI")
    _refused(b"\x89PNG\r\n\x1a\n" + bytes(32), "no SOI")


def test_refusals_by_patched_markers():
    g = _good()
    sof = _seg(g, 0xC0)[1]
    for code, words in [(0xC1, "SOF1"), (0xC3, r"SOF3 \(lossless\)"), (0xC9, "arithmetic"), (0xCA, "arithmetic")]:
        _refused(_patch(g, sof + 1, code), words)
    _refused(_patch(g, sof + 4, 12), "12-bit samples")
    _refused(_patch(_patch(g, sof + 5, 0), sof + 6, 0), r"height 0 \(.*DNL")
    _refused(_patch(g, sof + 11, 0x41), r"sampling factors 4x1 1x1 1x1")
    _refused(_patch(g, sof + 11, 0x12), r"sampling factors 1x2")
    _refused(_patch(g, sof + 14, 0x21), r"sampling factors 2x2 2x1")
    dqt = _seg(g, 0xDB)[1]
    _refused(_patch(g, dqt + 4, 0x10), "16-bit DQT")
    sos = _seg(g, 0xDA)[1]
    _refused(_patch(g, sos + 4, 1), "several scans")
    _refused(_patch(g, sos + 4 + 1 + 6, 1), "progressive")                        # Ss = 1
    dnl = b"\xff\xdc\x00\x04\x00\x10"
    _refused(g[:sos] + dnl + g[sos:], "DNL")
    # a second scan after the first one's data
    eoi = g.rindex(b"\xff\xd9")
    _refused(g[:eoi] + g[sos:], "second SOS")
    # Adobe APP14: transform 1 is YCbCr and passes, transform 0 says the samples are RGB
    adobe = lambda t: b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t])
    assert ops.jpeg_probe(g[:2] + adobe(1) + g[2:])["width"] == 16
    _refused(g[:2] + adobe(0) + g[2:], "Adobe transform 0")
    # missing tables
    m, off, n = _seg(g, 0xC4, 0)
    _refused(g[:off] + g[off + n:], "missing DC Huffman table 0")
    m, off, n = _seg(g, 0xC4, 1)
    _refused(g[:off] + g[off + n:], "missing AC Huffman table 0")
    m, off, n = _seg(g, 0xDB, 1)
    _refused(g[:off] + g[off + n:], "missing quantisation table 1")
    # a DHT whose counts overflow 256 symbols / whose codes overflow their length (DC luma: counts at +5 .. +20)
    m, off, n = _seg(g, 0xC4, 0)
    _refused(_patch(_patch(g, off + 5 + 15, 200), off + 5 + 14, 100), "overflow 256 symbols")
    counts = list(g[off + 5:off + 21])
    assert counts[0] == 0 and counts[2] >= 3
    _refused(_patch(_patch(g, off + 5, 3), off + 7, counts[2] - 3), "codes overflow their length")
    # a stream that ends inside a marker segment
    _refused(g[:dqt + 20], "ends inside marker segment 0xdb")
    _refused(g[:sof + 3], "ends inside marker segment 0xc0")
    # restart markers that do not fit the frame
    r = _good(33, 47, 2, restart_marker_blocks=1)
    first = r.index(b"\xff\xd0", _seg(r, 0xDA)[1])
    _refused(_patch(r, first + 1, 0xD3), "RST3 where RST0 is due")
    _refused(g[:_seg(g, 0xDA)[1] + _seg(g, 0xDA)[2] + 4] + b"\xff\xd0" + g[_seg(g, 0xDA)[1] + _seg(g, 0xDA)[2] + 4:], "without DRI")


def test_mutation_corpus_always_returns_a_status():
    """Truncation at every byte of the header and at 32 positions of the scan, 256 single-byte overwrites at seeded positions:
    every call returns (a dict or a ValueError with words), none crashes."""
    g = _good(33, 47, 1, restart_marker_blocks=3)
    m, off, n = _seg(g, 0xDA)
    scan = off + n
    cuts = list(range(scan + 1)) + [int(v) for v in np.linspace(scan + 1, len(g) - 1, 32)]
    rng = np.random.default_rng(11)
    pos, val = rng.integers(0, len(g), 256), rng.integers(0, 256, 256)
    corpus = [g[:c] for c in cuts] + [_patch(g, int(p), int(v)) for p, v in zip(pos, val)]
    ok = refused = 0
    for data in corpus:
        try:
            info = ops.jpeg_probe(data)
            assert 0 < info["width"] <= 65535 and 0 < info["height"] <= 65535 and info["intervals"] >= 1
            ok += 1
        except ValueError as exc:
            assert len(str(exc)) > len("jpeg_probe: ")
            refused += 1
    assert ok + refused == len(corpus) and refused >= scan - 2 and ok > 0


def test_iter_jpeg_frames_thumbnail_and_garbage():
    frames = [J.encode(J.make_image(16, 16, i), 90, 2, restart_marker_blocks=1) for i in range(3)]
    thumb = J.encode(J.make_image(8, 8, 9), 50, 2)
    app1 = b"\xff\xe1" + (len(thumb) + 8).to_bytes(2, "big") + b"Exif\x00\x00" + thumb         # a whole JPEG inside APP1
    with_thumb = frames[1][:2] + app1 + frames[1][2:]
    data = frames[0] + with_thumb + b"\x00\x00junk" + frames[2] + b"trailing garbage \xff\x00"
    got = list(V.iter_jpeg_frames(data))
    assert got == [frames[0], with_thumb, frames[2]]
    assert ops.jpeg_probe(got[1])["width"] == 16                                 # the thumbnail is skipped by its segment length
    assert list(V.iter_jpeg_frames(b"")) == [] and list(V.iter_jpeg_frames(b"no picture here")) == []
    cut = list(V.iter_jpeg_frames(frames[0] + frames[1][:100]))
    assert cut == [frames[0], frames[1][:100]]                                   # a cut-off picture is handed on as it is


def test_open_stream_routing():
    cfg = lambda url: StreamConfig(name="cam", url=url, warmup_seconds=0.0)
    for url in ("/data/a.mjpeg", "/data/a.MJPG", "file:///data/a.jpg", "clip.jpeg"):
        assert isinstance(V.open_stream(cfg(url)), V.MjpegStream), url
    for url in ("/data/a.mp4", "rtsp://cam/a.mjpeg", "/data/a.h264", "http://host/a.jpg"):
        assert type(V.open_stream(cfg(url))) is V.RocDecodeStream, url
    assert isinstance(V.open_stream(cfg("synthetic://64x48")), V.SyntheticNv12Stream)


def test_mjpeg_stream_errors_without_a_device(tmp_path):
    def opened(name, payload=None):
        path = tmp_path / name
        if payload is not None:
            path.write_bytes(payload)
        return V.MjpegStream(StreamConfig(name="door", url=str(path), warmup_seconds=0.0))
    with pytest.raises(RuntimeError, match="Unable to open stream door: .*missing.mjpeg does not exist"):
        opened("missing.mjpeg").open_sync()
    with pytest.raises(RuntimeError, match="Unable to open stream door: .*is empty"):
        opened("empty.mjpeg", b"").open_sync()
    with pytest.raises(RuntimeError, match="Unable to open stream door: .*no JPEG picture"):
        opened("text.mjpeg", b"hello").open_sync()
    with pytest.raises(RuntimeError, match=r"Unable to open stream door: first frame: .*SOF2 \(progressive\)"):
        opened("prog.jpg", _good(progressive=True)).open_sync()
    with pytest.raises(RuntimeError, match="Unable to open stream door: first frame is 17x13"):
        opened("odd.jpg", _good(17, 13)).open_sync()
    s = opened("missing2.mjpeg")
    assert s.next_surface() is None                                              # not open: a failed read, not an exception


def test_helper_decoder_equals_pillow_on_the_whole_grid():
    n = 0
    for name, data in J.grid():
        assert np.array_equal(J.decode(data)["rgb"], J.pillow_rgb(data)), name
        n += 1
    assert n == 252
    g = J.encode(J.make_image(19, 21, 3)[..., 0], 90)
    assert np.array_equal(J.decode(g)["rgb"], J.pillow_rgb(g))
    for data in (_good(optimize=True), _good(33, 47, 1, qtables=[list(range(1, 65)), [7] * 64]), _good(4, 9, 2), _good(3, 5, 1)):
        assert np.array_equal(J.decode(data)["rgb"], J.pillow_rgb(data))
