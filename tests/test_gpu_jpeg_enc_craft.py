"""K7, the device JPEG encoder, on images crafted in the coefficient domain (tests/jpeg_enc_craft.py): every (run, size) symbol of
both Annex-K AC tables, ZRL chains, blocks without EOB, every DC category in both signs across MCUs, restarts and dummy blocks,
the longest blocks an image gives, 0xFF bytes at lane 0 and lane 63 of a stuffing step, at both sides of a pass boundary and in the
pad byte -- what ``synth.make_bgr``'s smooth pictures leave to chance.  Every comparison is ``bytes ==`` against
``oracle/jpeg_oracle.py``; tests/test_jpeg_enc_craft_host.py shows on the CPU that the set reaches all this and that Pillow's
libjpeg agrees with the oracle on every image of it."""
import functools

import numpy as np
import pytest
import torch

from oracle import jpeg_oracle as J
from realtime_video_analytics_32streams_amd import ops, synth
from tests import jpeg_enc_craft as E

pytestmark = pytest.mark.gpu

SMOOTH = [(72, 40, 80), (17, 9, 100)]            # two of test_gpu_preview_batch.MIXED, mixed into the batch


@functools.lru_cache(maxsize=None)
def _case(name):
    """(host image, quality, the oracle's stream) of one crafted image: computed once, shared by every test, never modified."""
    bgr, q = E.crafted()[name]
    return bgr, q, J.encode(bgr, q)


@functools.lru_cache(maxsize=None)
def _smooth(w, h, q):
    bgr = synth.make_bgr(31 + w + q, w, h)
    bgr.setflags(write=False)
    return bgr, q, J.encode(bgr, q)


def _dev(bgr):
    return torch.tensor(bgr, device="cuda")


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert got == want, what


@pytest.fixture(scope="module")
def enc():
    e = ops.JpegBatchEncoder(len(E.NAMES) + len(SMOOTH), (E.MAX_W, E.MAX_H))
    yield e
    e.close()


@pytest.mark.parametrize("name", E.NAMES)
def test_crafted_image_is_the_oracles_bytes(name):
    bgr, q, want = _case(name)
    _same(ops.jpeg_encode_bgr(_dev(bgr), q), want, name)


def test_the_whole_set_in_one_batch_in_both_orders(enc):
    """All crafted images and two smooth ones as ONE launch set, forwards and backwards: every stream is the one encoded alone
    (the oracle's), whatever its slot and its neighbours -- 1 to 10 intervals, 1 to 3 passes, qualities 75 to 100 side by side."""
    cases = [(n, _case(n)) for n in E.NAMES]
    cases[3:3] = [(str(c), _smooth(*c)) for c in SMOOTH[:1]]
    cases[-2:-2] = [(str(c), _smooth(*c)) for c in SMOOTH[1:]]
    assert max(c[0].shape[1] for _, c in cases) == E.MAX_W and max(c[0].shape[0] for _, c in cases) == E.MAX_H
    for order in (cases, cases[::-1]):
        got = enc.encode([_dev(c[0]) for _, c in order], [c[1] for _, c in order])
        for (name, c), g in zip(order, got):
            _same(g, c[2], name)


@pytest.mark.parametrize("name", ["dc-steps", "dense-2-200x40"])
def test_row_pitch_and_unaligned_storage(name):
    """A pitch other than 3 w (a [h, w, 3] view of a [h, w + 5, 3] tensor) and storage that starts 1 and 3 bytes into an
    allocation: the same bytes as the contiguous image."""
    bgr, q, want = _case(name)
    h, w = bgr.shape[:2]
    wide = torch.full((h, w + 5, 3), 77, dtype=torch.uint8, device="cuda")
    view = wide[:, :w, :]
    view.copy_(_dev(bgr))
    assert view.stride(0) == 3 * (w + 5) and not view.is_contiguous()
    _same(ops.jpeg_encode_bgr(view, q), want, (name, "pitch"))
    for off in (1, 3):
        flat = torch.full((h * w * 3 + 4,), 77, dtype=torch.uint8, device="cuda")
        img = flat[off:off + h * w * 3].view(h, w, 3)
        img.copy_(_dev(bgr))
        assert img.data_ptr() - flat.data_ptr() == off and flat.data_ptr() % 4 == 0
        _same(ops.jpeg_encode_bgr(img, q), want, (name, "offset", off))
    e = ops.JpegBatchEncoder(2, (w, h))                               # ... and through the batch entry point, both at once
    try:
        got = e.encode([view, img], [q, q])
        _same(got[0], want, (name, "batch pitch"))
        _same(got[1], want, (name, "batch offset"))
    finally:
        e.close()


def test_repeated_encode_and_a_smaller_image_after_a_larger(enc):
    """The same image twice in a row on one encoder gives the same bytes, and a picture of one interval after one of ten carries no
    stale interval sizes, offsets or flags (the scratch is reused, never cleared between calls)."""
    big, small = _case("pinned-5068-176x160-q97"), _case("dense-0-16x16")
    for _ in range(2):
        _same(enc.encode([_dev(big[0])], [big[1]])[0], big[2], "big")
    _same(enc.encode([_dev(small[0])], [small[1]])[0], small[2], "small after big")
    sheet, edge = _case("sheet-chroma-q100-1"), _case("dc-edge-8x24")
    got = enc.encode([_dev(sheet[0]), _dev(big[0])], [sheet[1], big[1]])
    _same(got[0], sheet[2], "sheet"); _same(got[1], big[2], "big beside sheet")
    got = enc.encode([_dev(edge[0]), _dev(small[0])], [edge[1], small[1]])
    _same(got[0], edge[2], "edge after sheet"); _same(got[1], small[2], "small after big, slot 1")
    for c in (big, small, big):                                      # the per-context encoder of jpeg_encode_bgr likewise
        _same(ops.jpeg_encode_bgr(_dev(c[0]), c[1]), c[2], "single")
