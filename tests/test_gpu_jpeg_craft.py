"""K8 on the GPU on hand-built streams no encoder writes (tests/jpeg_craft.py): every way to select Huffman and quantisation tables,
the long-code path of the Huffman decoder, block shapes at the ends of their ranges, stuffed bytes wherever they can stand, more
restart intervals than one block of entropy lanes, each documented failure on its own, and the ends of the NV12 range.  BGR is
compared with Pillow's libjpeg-turbo and NV12 with the formulas of include/rva.h on the planes of tests/jpeg_ref.py, both with no
tolerance; tests/test_jpeg_craft_host.py pins jpeg_ref to Pillow on every stream used here and asserts, from the writer's facts,
that each stream has the property it is named for."""
import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from tests import jpeg_craft as K
from tests import jpeg_ref as J

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL.Image")


def _bgr(data):
    return J.pillow_rgb(data)[..., ::-1]


def _same(t, want):
    return t is not None and np.array_equal(t.cpu().numpy(), want)


@pytest.fixture(scope="module")
def dec():
    d = ops.JpegBatchDecoder(64, (256, 256), 1 << 16)
    yield d
    d.close()


def _bgr_equals_pillow(dec, streams):
    names = list(streams)
    got = dec.decode([streams[n][0] for n in names], "bgr")
    assert dec.status == [0] * len(names), [n for n, s in zip(names, dec.status) if s]
    for n, t in zip(names, got):
        assert _same(t, _bgr(streams[n][0])), n


def _nv12_equals_the_formulas(dec, streams):
    names = list(streams)
    got = dec.decode([streams[n][0] for n in names], "nv12")
    assert dec.status == [0] * len(names), [n for n, s in zip(names, dec.status) if s]
    out = {}
    for n, s in zip(names, got):
        y, uv = J.nv12_expected(J.decode(streams[n][0]))
        gy, guv = s.y.cpu().numpy(), s.uv.cpu().numpy()
        assert np.array_equal(gy, y) and np.array_equal(guv, uv), n
        out[n] = (gy, guv)
    return out


def test_table_selection(dec):
    """16x16 and 24x16, gray / 4:4:4 / 4:2:2 / 4:2:0: all components on tables (1, 1); luma (1, 0) with chroma (0, 1); Cb (0, 1) with
    Cr (1, 0); quantisation ids (2, 3, 1) with three different tables; every table defined twice, the second time differently;
    everything in one DHT and one DQT segment; the tables behind SOF0.  One batch per output format."""
    streams = K.selection_streams()
    assert len(streams) == 2 * 4 * 7
    _bgr_equals_pillow(dec, streams)
    _nv12_equals_the_formulas(dec, streams)


def test_segment_layouts(dec):
    """DRI twice, zero, above and at the MCU count; fill bytes; comments that hold markers; JFIF, Adobe, neither; any component ids."""
    _bgr_equals_pillow(dec, K.layout_streams())


def test_entropy_edges(dec):
    """Tables whose shortest code has 9 bits (the look-ahead table is empty) and tables with the 16-bit code 0xFFFE in front of 11
    (DC) and 10 (AC) value bits; a ZRL that lands exactly on 64; runs of 15; 63 non-zero ACs; an immediate EOB; 32 stuffed bytes and
    more, two in a row, as the last bytes of an interval in front of RSTn and of EOI; 0-bit padding; fill bytes in front of RSTn and
    EOI."""
    streams = K.entropy_streams()
    assert {"edges-nine-bit-dri-3", "edges-sixteen-bit-dri-None", "stuffed", "stuffed-fill", "stuffed-pad-0", "nine-bit-4:2:0"} <= set(streams)
    f = streams["stuffed"][1]
    assert f["ff00"] >= 32 and f["ff00_twice"] and {0, f["intervals"] - 1} <= set(f["ends_ff00"])
    assert streams["edges-sixteen-bit-dri-3"][1]["longest_code_value"] == 27
    _bgr_equals_pillow(dec, streams)
    _nv12_equals_the_formulas(dec, streams)


def test_more_intervals_than_one_block_of_lanes(dec):
    """72 and 40 restart intervals (k8_entropy gives a block 64 lanes: a second block with a partial wavefront, and blocks that
    leave before the barrier for the pictures with fewer) in one batch with a picture of one interval and a gray one, in both
    orders: every picture equals its single decode and Pillow."""
    streams = K.lane_streams()
    names = list(streams)
    assert [streams[n][1]["intervals"] for n in names] == [72, 40, 1, 8]
    singles = {}
    for n in names:
        singles[n] = dec.decode([streams[n][0]], "bgr")[0].cpu().numpy()
        assert dec.status == [0] and np.array_equal(singles[n], _bgr(streams[n][0])), n
    for order in (names, names[::-1], [names[2], names[0], names[3], names[1], names[0]]):
        got = dec.decode([streams[n][0] for n in order], "bgr")
        assert dec.status == [0] * len(order)
        for n, t in zip(order, got):
            assert _same(t, singles[n]), (order, n)
    _nv12_equals_the_formulas(dec, streams)


def test_each_documented_failure_on_its_own(dec):
    """k8_entropy documents what fails a picture: a code in no table, a run past 63, a ZRL past 64, an interval that runs dry, bytes
    left over.  One stream per condition, built by the writer, well-formed in everything else (the parser accepts each: the host
    test), in the middle of a batch of good pictures: status FAILED exactly, no output, the neighbours bit-identical to their single
    decodes, and the decoder as good as new on the next call.  Also a fill byte in front of a stuffed pair (FF FF 00) inside an
    interval, and ONE extra 00 byte in front of EOI: Pillow decodes that last stream, K8 fails it by its documented rule that a
    whole byte left over in an interval is a failure -- the strictness is the rule, not an accident."""
    bad = K.bad_streams()
    assert len(bad) == 7
    sel, lanes = K.selection_streams(), K.lane_streams()
    good = [sel["24x16-4:2:0-q-2-3-1"][0], lanes["72-intervals-4:4:4"][0], lanes["gray"][0], K.entropy_streams()["stuffed"][0]]
    want = [_bgr(d) for d in good]
    for name, (data, _) in bad.items():
        batch = good[:2] + [data] + good[2:]
        got = dec.decode(batch, "bgr")
        assert dec.status == [0, 0, N.RVA_JPEG_DEC_FAILED, 0, 0], (name, dec.status)
        assert got[2] is None and dec.errors[2] == "the entropy segment is damaged", name
        assert all(_same(got[i], want[j]) for i, j in ((0, 0), (1, 1), (3, 2), (4, 3))), name
        got = dec.decode(good, "bgr")
        assert dec.status == [0] * 4 and all(_same(t, w) for t, w in zip(got, want)), name
    # all of them in one batch, NV12: the flags are per picture
    batch = [d for d, _ in bad.values()] + [good[0]]
    got = dec.decode(batch, "nv12")
    assert dec.status == [N.RVA_JPEG_DEC_FAILED] * 7 + [0] and got[:7] == [None] * 7
    y, uv = J.nv12_expected(J.decode(good[0]))
    assert np.array_equal(got[7].y.cpu().numpy(), y) and np.array_equal(got[7].uv.cpu().numpy(), uv)


def test_nv12_reaches_both_ends_of_its_range(dec):
    """constant_blocks pictures in which every Y, Cb and Cr value 0..255 occurs: k8_luma601 / k8_chroma601 on their whole domain,
    through the 4:4:4 2x2 mean, the 4:2:2 row mean and the 4:2:0 copy."""
    streams = K.range_streams()
    assert list(streams) == ["range-4:4:4", "range-4:2:2", "range-4:2:0"]
    for name, (gy, guv) in _nv12_equals_the_formulas(dec, streams).items():
        assert gy.min() == 16 and gy.max() == 235 and len(np.unique(gy)) == 220, name
        for k in range(2):
            c = guv[:, k::2]
            assert c.min() == 16 and c.max() == 240 and len(np.unique(c)) == 225, name
    _bgr_equals_pillow(dec, streams)


def test_bgr_at_the_corners_of_the_colour_conversion(dec):
    """Y in {0, 128, 255} x Cb x Cr over 16 values each with 0 and 255 among them: every clamp of jdcolor.c's conversion."""
    data, _ = K.bgr_range_stream()
    got = dec.decode([data], "bgr")[0].cpu().numpy()
    want = _bgr(data)
    assert dec.status == [0] and np.array_equal(got, want)
    assert want.min() == 0 and want.max() == 255 and len({tuple(p) for p in want[::8, ::8].reshape(-1, 3)}) > 400


def test_rgb_samples_are_refused_in_a_batch(dec):
    """Component ids 'R','G','B' without JFIF or Adobe: libjpeg (so Pillow and cv2) takes the samples for RGB; K8 has no such path
    and says so instead of showing a YCbCr decode of them."""
    lay = K.layout_streams()
    good = [lay["rgb-ids-with-jfif"][0], lay["ids-7-33-200"][0], lay["rgb-ids-with-adobe-1"][0]]
    got = dec.decode([good[0], K.rgb_ids_stream(), good[1], good[2]], "bgr")
    assert dec.status == [0, N.RVA_JPEG_DEC_REFUSED, 0, 0] and got[1] is None
    assert "component ids 'R','G','B' without a JFIF or Adobe marker (RGB samples; YCbCr only)" in dec.errors[1]
    assert _same(got[0], _bgr(good[0])) and _same(got[2], _bgr(good[1])) and _same(got[3], _bgr(good[2]))
    with pytest.raises(ValueError, match="RGB samples"):
        ops.jpeg_decode_bgr(K.rgb_ids_stream())
