"""The crafted images K7 is held to on the GPU (tests/jpeg_enc_craft.py), without a GPU: ``facts`` -- the oracle's own coefficients,
code tables and block coder -- says that the set reaches what it was built for (every AC symbol of both Annex-K tables, ZRL chains,
blocks without EOB, every DC category in both signs per component, every stuffing fact of the kernel's 64-byte steps and 64-block
passes), and Pillow's libjpeg-turbo says that the oracle is right on every one of them: for a symbol no smooth picture uses, this
is the only check that the oracle's code for it is libjpeg's and not a shared misreading of Annex K."""
import io
import json
import pathlib

import numpy as np
import pytest

from oracle import jpeg_oracle as J
from tests import jpeg_enc_craft as E

ALL_AC = {(run, size) for run in range(16) for size in range(1, 11)}
ALL_DC = {(cat, sign) for cat in range(1, 12) for sign in (1, -1)} | {(0, 0)}
# (run, size) symbols the crafted set does not reach, by table: none.  Size 10 in chroma needs |Cb - 128| >= 91, outside the gamut
# at constant luma; the sheets let the luma follow the colour there (``_chroma_lut``), which reaches 120.
LUMA_LEFT_OUT = set()
CHROMA_LEFT_OUT = set()


@pytest.fixture(scope="module")
def found():
    """{name: facts} of the whole crafted set, computed once."""
    return {name: E.facts(img, q) for name, (img, q) in E.crafted().items()}


def _union(found, key, sub):
    out = set()
    for f in found.values():
        out |= f[key][sub]
    return out


def test_the_names_are_the_set():
    assert tuple(E.crafted()) == E.NAMES
    assert all(img.shape[0] <= 160 and img.shape[1] <= 512 for img, _ in E.crafted().values())


def test_every_ac_symbol_of_both_tables_is_coded(found):
    luma, chroma = _union(found, "ac", "luma"), _union(found, "ac", "chroma")
    print("luma AC symbols", len(luma & ALL_AC), "chroma AC symbols", len(chroma & ALL_AC))
    assert len(LUMA_LEFT_OUT) <= 2 and len(CHROMA_LEFT_OUT) <= 15
    assert ALL_AC - luma == LUMA_LEFT_OUT and ALL_AC - chroma == CHROMA_LEFT_OUT
    assert len(luma & ALL_AC) >= 158 and {s for s in ALL_AC if s[1] <= 9} <= luma
    assert len(chroma & ALL_AC) >= 145 and {s for s in ALL_AC if s[1] <= 7} <= chroma


def test_zrl_chains_and_both_ends_of_a_block(found):
    for tab in ("luma", "chroma"):
        assert {1, 2, 3} <= _union(found, "zrl", tab), tab
        assert sum(f["no_eob"][tab] for f in found.values()) > 0, tab              # zz[63] != 0: the block ends without EOB
        assert sum(f["eob_only"][tab] for f in found.values()) > 0, tab


def test_every_dc_category_in_both_signs_per_component(found):
    for comp in ("y", "cb", "cr"):
        assert found["dc-steps"]["dc"][comp] == ALL_DC, (comp, sorted(ALL_DC - found["dc-steps"]["dc"][comp]))
    for name in ("dc-edge-24x24", "dc-edge-8x24", "dc-edge-24x8"):                # a category-11 step behind a dummy block
        assert {c for c, _ in found[name]["dc"]["y"]} >= {0, 11}, name


def test_a_predictor_that_survived_a_restart_would_change_dc_steps():
    img, q = E.crafted()["dc-steps"]
    (cy, ccb, ccr), _ = J.coefficients(img, q)
    assert cy.shape[0] // 2 >= 3
    for my in range(1, cy.shape[0] // 2):
        for first, last in ((cy[2 * my, 0, 0], cy[2 * my - 1, -1, 0]), (ccb[my, 0, 0], ccb[my - 1, -1, 0]), (ccr[my, 0, 0], ccr[my - 1, -1, 0])):
            assert abs(int(first) - int(last)).bit_length() >= 9, (my, first, last)


@pytest.mark.parametrize("fact", E.STUFFING_FACTS)
def test_every_stuffing_fact_is_shown(found, fact):
    """Each fact by a pinned noise image found by a search on the CPU.  300 seeds of 192x16 and 100 of 176x16 at quality 100 gave
    all but the 0xFF that is the last complete byte of a non-final pass: that one turned up once in 10 020 intervals (150 s) of
    192x160 noise at quality 100 and 176x160 at quality 97, in the pinned seed 5068.  The pinned cases keep the geometry they were
    searched at: 176 px and wider (a second pass), 16 to 160 rows."""
    pinned = {n: f for n, f in found.items() if n.startswith("pinned-")}
    assert len(pinned) == len(E.pinned_stuffing_cases()) > 0
    for seed, w, h, q in E.pinned_stuffing_cases():
        assert w >= 176 and 16 <= h <= 160 and found[f"pinned-{seed}-{w}x{h}-q{q}"]["passes_per_interval"] >= 2
    shown = [n for n, f in pinned.items() if f["stuffing"][fact]]
    print(fact, shown)
    assert shown, fact


@pytest.mark.parametrize("name", E.NAMES)
def test_oracle_is_pinned_by_pillows_libjpeg_on_crafted_images(name):
    """The three assertions of test_jpeg_oracle_is_pinned_by_pillows_libjpeg: Pillow decodes the oracle's stream to exactly the
    pixels it decodes from its own encoding at the same quality and 4:2:0, with equal quantisation tables and size -- and it can
    only decode the oracle's stream at all if every Huffman code in it is the one libjpeg reads from the header's tables."""
    from PIL import Image
    bgr, q = E.crafted()[name]
    data = J.encode(bgr, q)
    mine = Image.open(io.BytesIO(data)); mine.load()
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, format="JPEG", quality=q, subsampling="4:2:0")
    ref = Image.open(io.BytesIO(buf.getvalue())); ref.load()
    assert mine.size == ref.size == (bgr.shape[1], bgr.shape[0])
    assert {k: list(v) for k, v in mine.quantization.items()} == {k: list(v) for k, v in ref.quantization.items()}
    assert np.array_equal(np.asarray(mine.convert("RGB")), np.asarray(ref.convert("RGB")))


def test_recorded_coverage_is_what_the_set_gives(found):
    """profiles/jpeg_enc_craft.json (tools/jpeg_enc_craft_report.py) is this set's measured coverage, not a claim.  The largest
    block is a record, not a threshold: K7's private buffer holds 1728 bits, and full-contrast noise is as long as a block gets."""
    top = max(f["max_block_bits"] for f in found.values())
    alone = found["dense-0-16x16"]["max_block_bits"]
    print("largest block:", top, "bits; dense_noise(0, 16, 16) alone:", alone)
    assert top >= alone
    rec = json.loads((pathlib.Path(__file__).resolve().parents[1] / "profiles" / "jpeg_enc_craft.json").read_text())
    assert rec == json.loads(json.dumps(E.coverage(found)))
