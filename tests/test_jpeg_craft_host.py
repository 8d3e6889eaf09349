"""K8's host half and the K8 tests' own references on hand-built streams no encoder writes (tests/jpeg_craft.py), without a GPU:
tests/jpeg_ref.py equals Pillow's libjpeg-turbo bit for bit on every crafted stream the GPU tests use (which is what makes it and
Pillow trustworthy references there), the writer's facts say that each stream has the property it was built for, ``ops.jpeg_probe``
reads every layout of the marker segments, the colour space of three components follows libjpeg's rule, and planted faults in the
reference decoder show that the crafted streams see what the encoder-made grid cannot."""
import pathlib

import numpy as np
import pytest

from realtime_video_analytics_32streams_amd import ops
from tests import jpeg_craft as K
from tests import jpeg_ref as J

pytest.importorskip("PIL.Image")

GOLDEN = pathlib.Path(__file__).parent / "golden" / "jpeg_craft"
# the crafted layouts that seed tools/jpeg_parse_check.cpp (the stand-alone sanitizer run of the parser), as files
SEEDS = {"fill-bytes": K.layout_streams, "one-segment-after-sof": K.layout_streams, "com-and-app": K.layout_streams, "dri-twice": K.layout_streams,
         "rgb-ids-with-adobe-1": K.layout_streams, "16x16-4:2:0-redefined": K.selection_streams, "24x16-4:2:2-q-2-3-1": K.selection_streams,
         "stuffed-fill": K.entropy_streams, "edges-sixteen-bit-dri-3": K.entropy_streams}


@pytest.fixture(scope="module")
def pillow():
    """{name: Pillow's RGB} of every well-formed crafted stream, decoded once."""
    return {name: J.pillow_rgb(data) for name, (data, _) in K.good_streams().items()}


@pytest.fixture(scope="module")
def grid():
    return [(name, data, J.pillow_rgb(data)) for name, data in J.grid()]


def test_reference_equals_pillow_on_every_crafted_stream(pillow):
    good = K.good_streams()
    assert len(good) >= 90
    for name, (data, facts) in good.items():
        ref = J.decode(data)
        assert np.array_equal(ref["rgb"], pillow[name]), name
        assert -512 <= facts["idct_range"][0] and facts["idct_range"][1] <= 511, name


def test_the_streams_have_the_properties_they_were_built_for():
    e = K.entropy_streams()
    for dri in (None, 3):
        assert e[f"edges-sixteen-bit-dri-{dri}"][1]["longest_code"] == 16
        assert e[f"edges-sixteen-bit-dri-{dri}"][1]["longest_code_value"] == 16 + 11          # 0xFFFE and the 11 bits of a DC category 11
        assert e[f"edges-nine-bit-dri-{dri}"][1]["longest_code"] == 9
    assert K.codes(K.DC16)[11] == (0xFFFE, 16) and K.codes(K.AC16)[0x0A] == (0xFFFE, 16)          # ... and the 10 bits of run 0 / size 10
    assert min(n for _, n in K.codes(K.DC9).values()) == 9 and min(n for _, n in K.codes(K.AC9).values()) == 9
    # the edge blocks, read back: category 11 both ways, the ZRLs that land on 64, the runs of 15, the 63 ACs
    data = e["edges-sixteen-bit-dri-None"][0]
    scan = J.parse(data)["intervals"][0]
    zrl = format(K.codes(K.AC16)[0xF0][0], "03b")
    bits = "".join(format(b, "08b") for b in scan.replace(b"\xff\x00", b"\xff"))
    one = lambda v: "10" + ("1" if v > 0 else "0")                                               # AC16: run 0 / size 1 is code 10
    sign = lambda k: 1 if k % 3 else -1
    assert "".join(one(sign(k)) for k in range(1, 48)) + zrl + format(K.codes(K.DC16)[7][0], "08b") in bits     # 47 ACs, ONE ZRL, the next DC
    assert "".join(one(-sign(k)) for k in range(1, 32)) + zrl * 2 + format(K.codes(K.DC16)[6][0], "07b") in bits
    blocks = K.edge_blocks()[0].reshape(10, 64)[:, J.ZIGZAG]
    assert (blocks[7, 1:] != 0).all() and not blocks[8, 1:].any() and blocks[5, 16] and not blocks[5, 1:16].any()
    assert blocks[0, 0] - 0 == 2047 and blocks[1, 0] - blocks[0, 0] == -2047 and blocks[0, 1] == 1023 and blocks[1, 1] == -1023
    # stuffing: 32 pairs or more, two in a row, the last bytes of an interval in front of RSTn and in front of EOI
    for name in ("stuffed", "stuffed-fill"):
        data, f = e[name]
        assert f["ff00"] >= 32 and f["ff00_twice"] and 0 in f["ends_ff00"] and f["intervals"] - 1 in f["ends_ff00"], (name, f)
        assert data.count(b"\xff\x00") >= 32 and b"\xff\x00\xff\x00" in data
    assert b"\xff\x00\xff\xd0" in e["stuffed"][0] and e["stuffed"][0].endswith(b"\xff\x00\xff\xd9")
    assert b"\xff\x00\xff\xff\xff\xd0" in e["stuffed-fill"][0] and e["stuffed-fill"][0].endswith(b"\xff\x00\xff\xff\xff\xd9")
    assert e["stuffed-pad-0"][1]["scan_bits"] % 8 and e["stuffed-pad-0"][0] != e["stuffed"][0]
    lanes = K.lane_streams()
    assert [f["intervals"] for _, f in lanes.values()] == [72, 40, 1, 8]           # (the gray one: 15 MCUs in intervals of 2)
    # constant_blocks: exactly the values, every value of every plane
    for name, (data, _) in K.range_streams().items():
        planes = J.decode(data)["planes"]
        assert all(sorted(set(p[::8, ::8].ravel())) == list(range(256)) for p in planes), name
        assert all((p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8) == p[::8, ::8][:, None, :, None]).all() for p in planes), name
    planes = J.decode(K.bgr_range_stream()[0])["planes"]
    assert {(int(a), int(b), int(c)) for a, b, c in zip(*(p[::8, ::8].ravel() for p in planes))} == \
           {(y, cb, cr) for y in (0, 128, 255) for cb in K.CHROMA16 for cr in K.CHROMA16}


@pytest.mark.parametrize("name", list(K.LAYOUTS))
def test_probe_reads_every_layout(name):
    _, ri, n = K.LAYOUTS[name]
    data, facts = K.layout_streams()[name]
    assert ops.jpeg_probe(data) == dict(width=40, height=24, components=3, h_samp=2, v_samp=2, sampling="4:2:0", restart_interval=ri,
                                        intervals=n, mcus=6)
    assert facts["intervals"] == n and data.count(b"\xff\xd0") == (n > 1)                      # RST0 is there exactly when there are intervals


def test_probe_reads_the_table_selections_and_the_edges():
    for name, (data, facts) in {**K.selection_streams(), **K.entropy_streams(), **K.lane_streams()}.items():
        assert ops.jpeg_probe(data)["intervals"] == facts["intervals"], name
    info = ops.jpeg_probe(K.selection_streams()["24x16-4:2:2-q-2-3-1"][0])
    assert (info["width"], info["height"], info["sampling"], info["mcus"]) == (24, 16, "4:2:2", 4)


def test_colour_space_follows_libjpeg(pillow):
    """libjpeg's default_decompress_parms: JFIF says YCbCr; else Adobe's transform decides; else ids 1,2,3 are YCbCr, 'R','G','B' are
    RGB samples, anything else YCbCr.  Pillow shows what libjpeg decides."""
    rgb = K.rgb_ids_stream()
    with pytest.raises(ValueError, match=r"component ids 'R','G','B' without a JFIF or Adobe marker \(RGB samples; YCbCr only\)"):
        ops.jpeg_probe(rgb)
    ycc = J.decode(rgb)["rgb"]
    assert not np.array_equal(J.pillow_rgb(rgb), ycc), "Pillow took the samples for YCbCr: the refusal has no ground"
    assert np.array_equal(J.pillow_rgb(rgb), np.stack([p[:24, :40] for p in J.decode(rgb)["planes"]], -1))       # the samples ARE the picture
    for name in ("rgb-ids-with-jfif", "rgb-ids-with-adobe-1", "ids-0-1-2", "ids-7-33-200", "no-jfif", "adobe-1", "jfif-and-adobe-1"):
        data = K.layout_streams()[name][0]
        assert ops.jpeg_probe(data)["components"] == 3, name
        assert np.array_equal(pillow[name], J.decode(data)["rgb"]), name                        # accepted, and YCbCr is what Pillow decodes
    # an Adobe transform other than 1 stays refused, also beside JFIF, where libjpeg believes JFIF: the two contradict each other
    kw = dict(qtables={0: K.QA, 1: K.QB})
    for jfif in (False, True):
        data = K.write(40, 24, K.noise_blocks(40, 24, 3, (2, 2), seed=3), (2, 2), jfif=jfif, adobe=0, **kw)[0]
        with pytest.raises(ValueError, match="Adobe transform 0"):
            ops.jpeg_probe(data)


def test_the_parser_accepts_the_streams_that_fail_on_the_device():
    """Each is well-formed up to one fault in its entropy segment, which only the device reads.  One extra 00 byte in front of EOI
    is a stream Pillow decodes; K8 fails it by its documented rule (a whole byte left over in an interval)."""
    bad = K.bad_streams()
    assert list(bad) == ["code-in-no-table", "run-past-63", "zrl-past-64", "interval-runs-dry", "bytes-left-over", "ff-ff-00", "extra-00-before-eoi"]
    for name, (data, facts) in bad.items():
        assert ops.jpeg_probe(data)["intervals"] == facts["intervals"], name
    blocks = K.noise_blocks(32, 16, 1, None, seed=11)
    good = K.write(32, 16, blocks, td=(0,), ta=(0,), tq=(0,))
    assert bad["extra-00-before-eoi"][0] == good[0][:-2] + b"\x00\xff\xd9"
    assert np.array_equal(J.pillow_rgb(bad["extra-00-before-eoi"][0]), J.pillow_rgb(good[0]))
    assert bad["bytes-left-over"][0] == good[0][:-2] + b"\x55\xaa\xff\xd9"
    dry, facts = bad["interval-runs-dry"]
    assert good[1]["scan_bits"] - facts["scan_bits"] >= 16 and good[0].startswith(dry[:-2 - 1])          # a prefix: whole blocks are missing
    assert bad["ff-ff-00"][0].count(b"\xff\xff\x00") == 1 and K.entropy_streams()["stuffed"][0].count(b"\xff\xff\x00") == 0


# planted fault -> what it gets wrong.  Each is one line of tests/jpeg_ref.py (FAULTS) switched on.
MUTANTS = ["ac-by-dc-id", "q-min-c-1", "cb-cr-swapped", "first-definition", "first-of-segment", "zrl-64-error"]
SEEN_BY_THE_GRID = ["pred-kept", "search-15"]


def _differs(data, want, fault):
    try:
        return not np.array_equal(J.decode(data, fault)["rgb"], want)
    except (AssertionError, KeyError, IndexError):             # the mutant lost its way in the bits: a failed decode is a difference
        return True


def _small(pillow):
    return {name: (data, pillow[name]) for name, (data, _) in K.good_streams().items() if pillow[name].size <= 3 * 64 * 64}


@pytest.mark.parametrize("fault", MUTANTS)
def test_mutant_is_caught_by_the_crafted_streams_and_missed_by_the_grid(fault, pillow, grid):
    """A decoder that takes the AC table by the DC id, the quantisation table by min(c, 1), Cr's tables for Cb, the first definition
    of a table instead of the last, only the first table of a segment, or a ZRL that lands on 64 for an error differs from Pillow
    on a crafted stream and equals Pillow on all 252 streams of J.grid(): the grid cannot see these faults, the crafted streams do.
    Two more planted faults of the same kind, the DC prediction kept over a restart and the code search stopped at 15 bits, ARE seen
    by the grid (its restart intervals; Annex K's 16-bit codes at quality 90 and 100), so they are no evidence for the crafted
    streams and are not in this list: test_two_faults_the_grid_sees_as_well records that."""
    caught = [name for name, (data, want) in _small(pillow).items() if _differs(data, want, fault)]
    assert caught, fault
    expected = {"ac-by-dc-id": "16x16-4:2:0-luma-1-0-chroma-0-1", "q-min-c-1": "16x16-4:2:0-q-2-3-1", "cb-cr-swapped": "16x16-4:2:0-cb-0-1-cr-1-0",
                "first-definition": "16x16-4:2:0-redefined", "first-of-segment": "16x16-4:2:0-one-segment", "zrl-64-error": "edges-annex-k-dri-None"}
    assert expected[fault] in caught                              # the stream DESIGN.md's table names for it
    assert len(grid) == 252
    for name, data, want in grid:
        assert not _differs(data, want, fault), (fault, name)


@pytest.mark.parametrize("fault", SEEN_BY_THE_GRID)
def test_two_faults_the_grid_sees_as_well(fault, pillow, grid):
    assert any(_differs(data, want, fault) for data, want in _small(pillow).values())
    assert any(_differs(data, want, fault) for _, data, want in grid)


def test_the_sanitizer_seeds_are_the_writers_streams():
    """tests/golden/jpeg_craft/*.jpg feed tools/jpeg_parse_check.cpp; they are what the writer makes today."""
    assert sorted(p.stem for p in GOLDEN.glob("*.jpg")) == sorted(n.replace(":", "") for n in SEEDS)
    for name, source in SEEDS.items():
        assert (GOLDEN / (name.replace(":", "") + ".jpg")).read_bytes() == source()[name][0], name
