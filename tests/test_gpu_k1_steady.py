"""The steady-state K1 (``k1_ratio_content``: content rectangle only, the letterbox border left as the buffer holds it)
against the oracle, bit for bit, and the detector bookkeeping that decides when it may run.

Every kernel-level case runs one protocol on a tensor poisoned with NaN bit patterns no pixel can produce:

1. S0 everywhere, full launch on frames A: the whole tensor is oracle(A);
2. S1 on the content rectangle, content launch on frames B: the whole tensor is oracle(B) (the border is the full
   launch's 114/255 and no S1 is left: every content pixel was written);
3. S2 on the border, S1 on the rectangle, content launch on frames C: the rectangle is oracle(C), every border element
   is still S2 (nothing is written outside the rectangle);
4. one full launch, then content launches on frames D, E, F: the whole tensor is the oracle after each one.

Frames differ per image (seed) and per launch (``tick``).  Needs a real MI355X.

What each case reaches in ``rva_preprocess.hip`` (content launches; the full launches of the protocol run ``k1_ratio``):

  k1_ratio_content<R, half|float, 2>   R = 1, 2, 3, 4, 6: every_ratio (fp16 and fp32); R = 3 also odd_geometry 1920x1086
                                       (top 139), other_rectangles, pitches, 8-byte-aligned planes, batch sizes n = 1;
                                       R = 1 batch sizes n = 64, 70; R = 2 other_rectangles 640x1280
  k1_ratio_content<R, half|float, 1>   R = 2, 4, 6: odd_geometry (new_h 361).  An odd R cannot give an odd new_h from an
                                       even NV12 height, so RPT 1 exists for even R only
  k1_ratio_content<3, half, 2, NT>     NT = 1, 2, 3: non_temporal_forms (plain and event launch); 720p and fp32 under the
                                       same switch take the plain form
  hipExtLaunchKernelGGL content form   with_dispatch_events (R = 3 and R = 2, fp16); non_temporal_forms (NT forms)
  content_only -> full launch          R = 5 (no content instantiation, no k1_ratio: k1_generic), 1000x700, pitch % 8 != 0,
                                       planes at byte offset 4 (k1_generic)
  k1_ratio<R, half, 16, false>         R = 3 and R = 2: 16_pixels_per_lane (RVA_K1_PX=16)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops, synth
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig
from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
from realtime_video_analytics_32streams_amd.gates import rasterize_polygons
from realtime_video_analytics_32streams_amd.video_stream import FramePacket

pytestmark = pytest.mark.gpu
DEV = "cuda"

# NaN payloads no pixel can produce (S0, S1, S2): integer views, compared bit for bit
SENTINELS = {True: (0x7E01, 0x7E02, 0x7E03), False: (0x7FC00001, 0x7FC00002, 0x7FC00003)}


def _pitch256(w):
    return ((w + 255) // 256) * 256


@functools.lru_cache(maxsize=256)
def _frame(w, h, pitch, img, tick):
    return synth.make_nv12(synth.SEED_BASE + 1000 * img, w, h, pitch, tick=tick)


@functools.lru_cache(maxsize=256)
def _want(w, h, pitch, img, tick, tw, th, half):
    """Oracle bits of one frame (uint16 / uint32 view) and its letterbox meta."""
    y, uv = _frame(w, h, pitch, img, tick)
    out, meta = orc.preprocess_nv12(y, uv, w, h, tw, th, half)
    bits = out.view(np.uint16 if half else np.uint32)
    bits.setflags(write=False)
    return bits, meta


def _upload(a, offset):
    """Device copy of a host plane; with ``offset`` a view at that byte offset of a larger allocation (the planes end
    where the allocation ends, so every read stays inside it)."""
    if offset == 0:
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    buf = torch.empty(a.size + offset, dtype=torch.uint8, device=DEV)
    v = buf[offset:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def _surface(y, uv, w, h, offset=0, mask=None):
    return ops.Nv12Surface(_upload(y, offset), _upload(uv, offset), w, h, mask=mask)


def _bits(t):
    return t.cpu().numpy().view(np.uint16 if t.dtype == torch.float16 else np.uint32)


def _same(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    i = tuple(int(v) for v in bad[0])
    raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; first at [img, c, y, x] = {i}: "
                         f"got {int(got[i]):#x}, want {int(want[i]):#x}")


def _rect(w, h, tw, th):
    """Bool [th, tw]: the content rectangle of the letterbox."""
    lb = orc.letterbox(w, h, tw, th)
    (nw, nh), (left, top) = lb["new"], lb["pad"]
    m = np.zeros((th, tw), bool)
    m[top:top + nh, left:left + nw] = True
    return m


def _protocol(w, h, *, n=2, half=True, dst=(640, 640), pitch=None, offset=0, ctx=None, arm=None, fallback=False):
    """The four steps of the module docstring.  ``fallback``: ``content_only`` cannot take the content kernel here
    (geometry, pitch or alignment), so every launch must be a full one -- the border is rewritten, S2 does not survive."""
    th, tw = dst
    pitch = pitch or _pitch256(w)
    ctx = ctx or ops.context()
    s0, s1, s2 = SENTINELS[half]
    out = torch.empty((n, 3, th, tw), dtype=torch.float16 if half else torch.float32, device=DEV)
    ints = out.view(torch.int16 if half else torch.int32)
    rect = _rect(w, h, tw, th)
    rect_d = torch.from_numpy(rect).to(DEV)
    assert rect.any()

    def launch(tick, content):
        surfs = [_surface(*_frame(w, h, pitch, i, tick), w, h, offset) for i in range(n)]
        if offset:
            assert all(s.y.data_ptr() % 16 == offset % 16 and s.uv.data_ptr() % 16 == offset % 16 for s in surfs)
        if arm is not None:
            arm(ctx)
        res, meta = ops.preprocess_nv12(surfs, dst, half=half, out=out, ctx=ctx, content_only=content)
        assert res is out
        wants = [_want(w, h, pitch, i, tick, tw, th, half) for i in range(n)]
        assert meta.as_meta() == wants[0][1], (tick, content)
        return np.stack([b for b, _ in wants])

    tag = f"{w}x{h}->{tw}x{th} {'fp16' if half else 'fp32'} n={n} pitch={pitch} offset={offset}"
    ints.fill_(s0)                                                               # 1
    want = launch(0, False)
    _same(_bits(out), want, f"{tag}: full launch")
    ints.masked_fill_(rect_d, s1)                                                # 2
    want = launch(1, True)
    _same(_bits(out), want, f"{tag}: content launch after a full one")
    ints.fill_(s2)                                                               # 3
    ints.masked_fill_(rect_d, s1)
    want = launch(2, True)
    if not fallback:
        want = np.where(rect, want, np.array(s2, want.dtype))
    _same(_bits(out), want, f"{tag}: content launch into a poisoned border" + (" (fallback: full launch)" if fallback else ""))
    want = launch(2, False)                                                      # 4
    _same(_bits(out), want, f"{tag}: full launch restoring the border")
    for tick in (3, 4, 5):
        want = launch(tick, True)
        _same(_bits(out), want, f"{tag}: content launch {tick - 2} of 3 after the restore")
    return out


# ------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("half", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("wh", [(640, 360), (1280, 720), (1920, 1080), (2560, 1440), (3840, 2160)],
                         ids=["R1-640x360", "R2-1280x720", "R3-1920x1080", "R4-2560x1440", "R6-3840x2160"])
def test_content_kernel_every_ratio_two_rows_per_thread(wh, half):
    """Every R of ``launch_content`` with an even ``new_h`` (360: RPT 2, rows half a frame apart)."""
    w, h = wh
    _protocol(w, h, half=half, n=32 if wh == (1920, 1080) else 2)


@pytest.mark.parametrize("half", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("wh", [(1280, 722), (2560, 1444), (3840, 2166), (1920, 1086)],
                         ids=["R2-rpt1-1280x722", "R4-rpt1-2560x1444", "R6-rpt1-3840x2166", "R3-oddtop-1920x1086"])
def test_content_kernel_odd_geometry(wh, half):
    """``new_h`` 361 (RPT 1, top 139; an even R divides an even height into an odd one) and ``new_h`` 362 with top 139."""
    w, h = wh
    lb = orc.letterbox(w, h, 640, 640)
    assert lb["pad"][1] == 139 and lb["new"][1] == (362 if wh == (1920, 1086) else 361)
    _protocol(w, h, half=half)


@pytest.mark.parametrize("half", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", [((960, 1920), (640, 640)), ((640, 1280), (640, 640)), ((1920, 1920), (640, 640)),
                                  ((1248, 702), (416, 416)), ((3840, 2160), (1280, 1280))],
                         ids=["R3-left160-960x1920", "R2-left160-640x1280", "R3-noborder-1920x1920",
                              "R3-1248x702-to-416", "R3-3840x2160-to-1280"])
def test_content_kernel_other_rectangles(case, half):
    """Pillarbox (``left`` != 0), no border at all, other detector input sizes."""
    (w, h), dst = case
    _protocol(w, h, half=half, dst=dst)


@pytest.mark.parametrize("pitch", [1920, 1928, 2048], ids=["pitch=width", "pitch=width+8", "pitch=256-multiple"])
def test_content_kernel_pitches(pitch):
    _protocol(1920, 1080, pitch=pitch)


def test_content_kernel_planes_8_byte_aligned():
    """Y / UV planes 8-byte but not 16-byte aligned: still the integer-ratio path (8-byte loads)."""
    _protocol(1920, 1080, offset=8)


@pytest.mark.parametrize("n,wh", [(1, (1920, 1080)), (64, (640, 360)), (70, (640, 360))],
                         ids=["n1", "n64", "n70-two-launches"])
def test_content_kernel_batch_sizes(n, wh):
    """``RVA_MAX_BATCH`` (64) frames in one launch, and 70: ``ops.preprocess_nv12`` launches twice, the second at out[64]."""
    assert N.RVA_MAX_BATCH == 64
    _protocol(*wh, n=n)


@pytest.mark.parametrize("case", [dict(w=3200, h=1800), dict(w=1000, h=700), dict(w=1920, h=1080, pitch=1924),
                                  dict(w=1920, h=1080, offset=4)],
                         ids=["R5-3200x1800", "generic-1000x700", "pitch1924", "planes-at-offset-4"])
def test_content_only_without_the_fast_path_is_a_full_launch(case):
    """``content_only=True`` where the content kernel does not apply falls back to a full launch: oracle bits, border
    rewritten."""
    _protocol(**case, fallback=True)


def _event_armer():
    pairs = []

    def arm(ctx):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        b.record()                                       # torch creates the hipEvents at the first record()
        torch.cuda.synchronize()
        assert N.lib().rva_profile_next_preprocess(ctx.handle, a.cuda_event, b.cuda_event) == N.RVA_OK
        pairs.append((a, b))
    return arm, pairs


@pytest.mark.parametrize("wh", [(1920, 1080), (1280, 720)], ids=["1920x1080", "1280x720"])
def test_content_kernel_with_dispatch_events(wh):
    """The ``hipExtLaunchKernelGGL`` form bench.py times K1 with (``rva_profile_next_preprocess`` before each launch)."""
    arm, pairs = _event_armer()
    _protocol(*wh, n=32 if wh == (1920, 1080) else 2, arm=arm)
    torch.cuda.synchronize()
    assert len(pairs) == 7 and all(a.elapsed_time(b) >= 0.0 for a, b in pairs)


@pytest.mark.parametrize("nt", [1, 2, 3], ids=["nt1-loads", "nt2-stores", "nt3-both"])
def test_content_kernel_non_temporal_forms(nt, monkeypatch):
    """``RVA_K1_NT`` (read once per context, so a fresh one): the non-temporal forms exist for R = 3 fp16; 720p (R = 2) and
    fp32 take the plain form under the same switch."""
    monkeypatch.setenv("RVA_K1_NT", str(nt))
    ctx = N.Context(torch.cuda.current_device())
    try:
        _protocol(1920, 1080, n=32, ctx=ctx)
        arm, _ = _event_armer()
        _protocol(1920, 1080, n=2, ctx=ctx, arm=arm)
        _protocol(1280, 720, ctx=ctx)
        _protocol(1920, 1080, half=False, ctx=ctx)
    finally:
        torch.cuda.synchronize()
        ctx.close()


@pytest.mark.parametrize("wh", [(1920, 1080), (1280, 720)], ids=["R3-1920x1080", "R2-1280x720"])
def test_full_kernel_16_pixels_per_lane(wh, monkeypatch):
    """Opt-in ``RVA_K1_PX=16`` (``k1_ratio<R, half, 16>``, 16-byte loads): full launches, and the content launches that
    follow them."""
    monkeypatch.setenv("RVA_K1_PX", "16")
    ctx = N.Context(torch.cuda.current_device())
    try:
        _protocol(*wh, n=32 if wh == (1920, 1080) else 2, ctx=ctx)
    finally:
        torch.cuda.synchronize()
        ctx.close()


# ------------------------------------------------------------------------------------------ detector level
class _Head:
    """``infer_fn`` stub: records the input tensor of every call, returns an empty head (no network is built)."""

    def __init__(self):
        self.seen = []

    def __call__(self, t):
        self.seen.append(t.clone())
        return torch.zeros((t.shape[0], 84, 8400), dtype=torch.float32, device=t.device)


@pytest.fixture
def k1_flags(monkeypatch):
    """``content_only`` of every ``ops.preprocess_nv12`` call the detector makes."""
    flags = []
    real = ops.preprocess_nv12

    def spy(*a, **kw):
        flags.append(bool(kw.get("content_only", False)))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "preprocess_nv12", spy)
    return flags


def _roi(w, h):
    return rasterize_polygons([[(w // 8, h // 6), (w * 3 // 4, h // 5), (w * 2 // 3, h * 5 // 6), (w // 5, h * 3 // 4)]], w, h)


def _tick_frames(kind, w, h, n, tick, half):
    """Frames of one detector call and the oracle bits of its input tensor."""
    if kind == "bgr":
        frames = [synth.make_bgr(100 * tick + i, w, h) for i in range(n)]
        want = [orc.preprocess_bgr(f, 640, 640, half)[0] for f in frames]
        return frames, np.stack(want).view(np.uint16 if half else np.uint32)
    pitch = _pitch256(w)
    frames, want = [], []
    for i in range(n):
        y, uv = _frame(w, h, pitch, i, tick)
        if kind == "mask" and i == 1:                  # one surface of the tick carries an ROI mask
            mask = _roi(w, h)
            frames.append(_surface(y, uv, w, h, mask=torch.from_numpy(mask).to(DEV)))
            masked = orc.nv12_to_bgr(y, uv, w, h) & (mask[..., None] // 255 * 255)     # cv2.bitwise_and(frame, frame, mask)
            want.append(orc.preprocess_bgr(masked, 640, 640, half)[0].view(np.uint16 if half else np.uint32))
        else:
            frames.append(_surface(y, uv, w, h))
            want.append(_want(w, h, pitch, i, tick, 640, 640, half)[0])
    return frames, np.stack(want)


HD = (1920, 1080)
# steps: (frame kind, (w, h), batch, detector slot, content_only expected of the call -- None: no NV12 call)
SEQUENCES = {
    "steady-1080p": [("nv12", HD, 4, 0, False), ("nv12", HD, 4, 0, True), ("nv12", HD, 4, 0, True)],
    "640x480-between": [("nv12", HD, 4, 0, False), ("nv12", (640, 480), 4, 0, False), ("nv12", HD, 4, 0, False),
                        ("nv12", HD, 4, 0, True)],
    "720p-between": [("nv12", HD, 4, 0, False), ("nv12", (1280, 720), 4, 0, False), ("nv12", HD, 4, 0, False)],
    "roi-mask-tick": [("nv12", HD, 4, 0, False), ("nv12", HD, 4, 0, True), ("mask", HD, 4, 0, False),
                      ("nv12", HD, 4, 0, False), ("nv12", HD, 4, 0, True)],
    "host-bgr-tick": [("nv12", HD, 4, 0, False), ("bgr", HD, 4, 0, None), ("nv12", HD, 4, 0, False), ("nv12", HD, 4, 0, True)],
    "batch-4-3-4": [("nv12", HD, 4, 0, False), ("nv12", HD, 3, 0, False), ("nv12", HD, 4, 0, True)],
    "second-slot": [("nv12", HD, 4, 0, False), ("nv12", HD, 4, 0, True), ("nv12", HD, 4, 1, False), ("nv12", HD, 4, 1, True),
                    ("nv12", HD, 4, 0, True)],
}


@pytest.mark.parametrize("half", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("seq", list(SEQUENCES), ids=list(SEQUENCES))
def test_detector_border_bookkeeping(seq, half, k1_flags):
    """``HipYoloDetector._preprocess`` runs the content kernel only into a buffer whose border holds this geometry's pad:
    after every call the tensor the network receives is the oracle's, and the full / content choice is the expected one
    (per buffer: batch size and slot; keyed on the frame size; a masked or host-frame tick resets it)."""
    head = _Head()
    cfg = DetectorConfig(model_path="yolov8n.pt", backend="hip", model_type="yolov8", half=half, warmup=False,
                         confidence_threshold=0.25, hip_engine="auto" if half else "plan")
    det = HipYoloDetector(cfg, infer_fn=head)
    sc = StreamConfig(name="cam0", url="synthetic://1920x1080", warmup_seconds=0.0)
    for tick, (kind, (w, h), n, slot, content) in enumerate(SEQUENCES[seq]):
        frames, want = _tick_frames(kind, w, h, n, tick, half)
        before = len(k1_flags)
        with torch.inference_mode():                   # the three stages as the runner drives them, in the step's slot
            pre = det.stage_pre([FramePacket(stream=sc, frame=f, frame_id=tick, timestamp=0.0) for f in frames], slot)
            det.stage_post(det.stage_net(pre), pre)
        assert k1_flags[before:] == ([] if content is None else [content]), (seq, tick)
        assert len(head.seen) == tick + 1
        _same(_bits(head.seen[-1]), want, f"{seq} {'fp16' if half else 'fp32'} tick {tick} ({kind} {w}x{h} n={n} slot {slot})")
