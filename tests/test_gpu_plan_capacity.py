"""One YOLOv8 plan serves every image count up to its capacity (``rva_yolov8_plan_run_n`` / ``_run_lanes_n`` / ``_run_range_n``,
include/rva.h; ``hip_plan_capacity``, config.py): images ``[0, n)`` of a partial run carry the bits of the same images of a full run
on the same kind of plan, nothing behind them is written, the static-row bookkeeping counts primed images, and a detector or a
pipeline whose live-stream count changes from tick to tick keeps one plan per slot and the results of the full batch."""
import copy
import ctypes as C
import logging
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
from realtime_video_analytics_32streams_amd.engine import FusedYoloV8
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
from realtime_video_analytics_32streams_amd.tracker import IouTracker
from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream
from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density

pytestmark = pytest.mark.gpu

SENTINEL = 0x7A5A           # fp16 bit pattern (51008.0): no head value comes near it (boxes stay below 1024, scores below 1)
SENTINEL32 = 0x7F7A5A5A     # as int32: an fp32 NaN pattern no kernel produces
PLANS = {"s": ("s", 3, (256, 64)), "n": ("n", 4, (256, 96))}          # the small plans of test_gpu_static_rows.py, as capacities
WINDOW = (96, 160)
BORDER = 0.447
_ENV = ("RVA_PLAN_NO_STATIC_ROWS", "RVA_PAIR32", "RVA_NO_STEM2", "RVA_NO_CIN_PAD", "RVA_TUNE_LAYER_OVERLAP", "RVA_SERIAL_HEADS")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _fill(t):
    _bits(t).fill_(SENTINEL if t.dtype == torch.float16 else SENTINEL32)


def _untouched(t) -> bool:
    return bool((_bits(t) == (SENTINEL if t.dtype == torch.float16 else SENTINEL32)).all())


def _rand(B, hw, seed, dtype=torch.float16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((B, 3, *hw), device="cuda", generator=g).to(dtype)


def _input(B, hw, top, bottom, seed, border=BORDER):
    x = torch.full((B, 3, *hw), border, dtype=torch.float16, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    x[:, :, top:bottom] = torch.rand((B, 3, bottom - top, hw[1]), device="cuda", generator=g).half()
    return x


def _build(scale, B, hw, net=None, **kw):
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    try:
        return FusedYoloV8(net if net is not None else build_detector_net(scale, seed=3), B, hw=hw, autotune=False, **kw)
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module", params=list(PLANS))
def plan_pair(request):
    """``a`` only ever runs full batches (the reference, computed once per input), ``b`` runs the partial ones."""
    scale, B, hw = PLANS[request.param]
    net = build_detector_net(scale, seed=3)
    return scale, B, hw, net, _build(scale, B, hw, net), _build(scale, B, hw, net)


def _check_partial(b, x, n, want, what):
    """Run ``b`` on the leading ``n`` images of ``x`` into a sentinel-filled output: images [0, n) carry ``want``'s bits, the rest
    keeps the sentinel."""
    _fill(b.out)
    got = b(x[:n])
    torch.cuda.synchronize()                               # a HIP error ends the case here
    assert tuple(got.shape) == (n,) + tuple(b.out.shape[1:]) and got.data_ptr() == b.out.data_ptr(), what
    res = b.result()
    assert tuple((res.head if isinstance(res, ops.SplitHead) else res).shape) == tuple(got.shape), what
    assert torch.equal(_bits(b.out[:n]), _bits(want[:n])), ("images [0, n) differ from the full run", what)
    assert _untouched(b.out[n:]), ("images >= n of the output were written", what)


def _partial_rounds(a, b, B, hw, ns, tag):
    x, y = _rand(B, hw, 1), _rand(B, hw, 2)
    want = a(x).clone()
    torch.cuda.synchronize()
    for n in ns:
        b(x)                                               # the buffers behind image n - 1 hold this input's activations
        _check_partial(b, x, n, want, (tag, n, "after a full run on the same data"))
        b(y)                                               # ... another input's
        _check_partial(b, x, n, want, (tag, n, "other images hold other data"))
        xi = x.clone()
        xi[n:] = float("inf")                              # the input behind the run is not read at all
        _check_partial(b, xi, n, want, (tag, n, "+Inf in the input images >= n"))


def test_partial_run_equals_the_rows_of_the_full_run(plan_pair):
    """Case 1: every n below the capacity with variant 0 on every step, then n = 1 and n = B - 1 with every variant forced on
    every tunable step that takes it (the same selection in the reference plan: bit-equality is per kernel)."""
    scale, B, hw, net, a, b = plan_pair
    for _, cell, _ in a._tunable + b._tunable:
        cell["variant"] = 0
    _partial_rounds(a, b, B, hw, range(1, B), "variant 0")
    forced = 0
    try:
        for v in range(1, int(N.lib().rva_conv_num_variants()) + 1):
            took = 0
            for (la, ca, _), (lb, cb, _) in zip(a._tunable, b._tunable):
                ok = lb(_stream(), v) == N.RVA_OK          # RVA_ERR_ARG through launch_tunable: the step keeps 0
                ca["variant"] = cb["variant"] = v if ok else 0
                took += ok
            forced += took
            if took:
                _partial_rounds(a, b, B, hw, sorted({1, B - 1}), f"variant {v} on {took} steps")
    finally:
        for _, cell, _ in a._tunable + b._tunable:
            cell["variant"] = 0
    assert forced > 0, "no step of this plan took a non-zero variant in any round"


@pytest.mark.parametrize("hw", [(256, 256), (512, 512)], ids=["256x256", "512x512"])
def test_variant_0_chooses_from_the_capacity(hw):
    """Case 2: YOLOv8s with capacity 8, n = 1, variant 0 everywhere.  Read off v_auto's size tests (256 CUs): at 256 x 256 none of
    them separates a batch of 1 from a batch of 8 (3x3 stride 1: M * Cout < 20 000 000 and M < 100 000 for both; b2.cv2, the one
    1x1 with Cin = 96 that bypasses the gather tile, has ceil(M / 256) * (cpad / 64) = 128 and 16, both below 2 * num_cus = 512),
    so that size is the control.  At 512 x 512 b2.cv2 (96 -> 64, 1x1, 128 x 128) flips on `t256 * (cpad / 64) >= 2 * num_cus`:
    t256 = 8 * 128 * 128 / 256 = 512 at the capacity -> res<64,64> (variant 5), t256 = 64 for one image -> res<64,32> (variant 6)
    had the choice been made from n."""
    B = 8
    net = build_detector_net("s", seed=3)
    a, b = _build("s", B, hw, net), _build("s", B, hw, net)
    x = _rand(B, hw, 5)
    want = a(x).clone()
    b(_rand(B, hw, 6))
    _check_partial(b, x, 1, want, ("capacity 8", hw))


def _call(plan, mode, x, n, out=None, sides=None):
    L, h = N.lib(), plan.handle
    xin, o = C.c_void_p(x.data_ptr()), C.c_void_p((plan.out if out is None else out).data_ptr())
    if mode == "run":
        return [L.rva_yolov8_plan_run_n(h, xin, o, n, _stream())]
    if mode == "lanes":
        return [L.rva_yolov8_plan_run_lanes_n(h, xin, o, n, _stream(), C.c_void_p(sides[0].cuda_stream), C.c_void_p(sides[1].cuda_stream))]
    return [L.rva_yolov8_plan_run_range_n(h, xin, o, n, 0, plan.quiet_step, _stream()),
            L.rva_yolov8_plan_run_range_n(h, xin, o, n, plan.quiet_step, plan.n_launches, _stream())]


def test_lanes_and_range_give_the_bits_of_run_n(plan_pair):
    """Case 3: the three run entry points, every n up to the capacity."""
    scale, B, hw, net, a, b = plan_pair
    sides = (torch.cuda.Stream(), torch.cuda.Stream())
    x = _rand(B, hw, 7)
    want = a(x).clone()
    for n in range(1, B + 1):
        for mode in ("run", "lanes", "range"):
            _fill(b.out)
            assert _call(b, mode, x, n, sides=sides) == [N.RVA_OK] * (2 if mode == "range" else 1), (mode, n)
            torch.cuda.synchronize()
            assert torch.equal(_bits(b.out[:n]), _bits(want[:n])) and _untouched(b.out[n:]), (mode, n)


def test_fp32_plan_partial_run():
    """Case 4: YOLOv8n, capacity 2 at 64 x 64, n = 1."""
    hw, net = (64, 64), build_detector_net("n", seed=3)
    a, b = _build("n", 2, hw, net, precision="fp32"), _build("n", 2, hw, net, precision="fp32")
    x = _rand(2, hw, 8, torch.float32)
    want = a(x).clone()
    b(_rand(2, hw, 9, torch.float32))
    _check_partial(b, x, 1, want, "fp32 plan")


def test_fp32_box_rows_partial_run():
    """Case 5: ``box_rows="fp32"``: the side tensor stays where the capacity puts it, its images [0, n) equal the full run's."""
    scale, B, hw = PLANS["s"]
    net = build_detector_net(scale, seed=3)
    a, b = _build(scale, B, hw, net, box_rows="fp32"), _build(scale, B, hw, net, box_rows="fp32")
    x = _rand(B, hw, 10)
    a(x)
    want, want32 = a.out.clone(), a.boxes32.clone()
    for n in range(1, B):
        b(_rand(B, hw, 11))
        _fill(b.boxes32)
        _check_partial(b, x, n, want, ("fp32 box rows", n))
        assert torch.equal(_bits(b.boxes32[:n]), _bits(want32[:n])) and _untouched(b.boxes32[n:]), n
        res = b.result()
        assert isinstance(res, ops.SplitHead) and res.head.shape[0] == n and res.boxes.shape[0] == n
        assert res.boxes.data_ptr() == b.boxes32.data_ptr()


def test_static_rows_count_primed_images(plan_pair):
    """Case 6: window (96, 160) of 256 rows against a plan that never windows."""
    scale, B, hw, net, a, _ = plan_pair
    top, bottom = WINDOW
    L = N.lib()
    primed = lambda p: int(L.rva_yolov8_plan_primed_images(p.handle))      # noqa: E731
    # (a) primed with the whole capacity, then partial runs on new content
    b = _build(scale, B, hw, net, static_rows=WINDOW)
    assert b.step_rows(0) != a.step_rows(0) and primed(b) == 0 and not b.primed
    b(_input(B, hw, top, bottom, 20))
    assert primed(b) == B and b.primed
    for n, seed in ((1, 21), (B - 1, 22)):
        x = _input(B, hw, top, bottom, seed)
        _check_partial(b, x, n, a(x).clone(), ("primed with B", n))
        assert primed(b) == B and b.primed
    # (b) primed with one image only: a larger run covers all rows of all its images (the never-run ones hold zeros)
    c = _build(scale, B, hw, net, static_rows=WINDOW)
    c(_input(B, hw, top, bottom, 23)[:1])
    assert primed(c) == 1 and c.primed                     # (the last run's image is covered)
    for seed in (24, 25):                                  # all rows, then windowed
        x = _input(B, hw, top, bottom, seed)
        want = a(x).clone()
        got = c(x)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want)), ("primed with 1, then B", seed)
        assert primed(c) == B
    # (c) what unprimes
    c.set_static_rows(top, bottom)
    assert primed(c) == 0 and not c.primed
    c(_input(B, hw, top, bottom, 26))
    assert primed(c) == B
    cell = c._tunable[0][1]
    cell["variant"] = cell["variant"]
    assert primed(c) == 0 and not c.primed


def test_bad_image_counts_are_refused_before_anything_is_launched(plan_pair):
    """Case 7."""
    scale, B, hw, net, a, b = plan_pair
    sides = (torch.cuda.Stream(), torch.cuda.Stream())
    x = _rand(B, hw, 12)
    _fill(b.out)
    for n in (0, -1, B + 1):
        for mode in ("run", "lanes", "range"):
            assert all(rc == N.RVA_ERR_ARG for rc in _call(b, mode, x, n, sides=sides)), (mode, n)
    torch.cuda.synchronize()
    assert _untouched(b.out)
    with pytest.raises(AssertionError):
        b(torch.cat([x, x[:1]]))


def test_one_capture_of_a_partial_run(plan_pair):
    """Case 8: ``_run_n`` with n = B - 1 recorded on a single stream after an eager run of the same n, replayed once."""
    scale, B, hw, net, a, b = plan_pair
    n = B - 1
    x = _rand(B, hw, 13)
    lanes = b.concurrent_heads
    b.concurrent_heads = False                             # rva_yolov8_plan_run_n, one stream
    try:
        want = b(x[:n]).clone()
        torch.cuda.synchronize()
        before = int(N.lib().rva_yolov8_plan_primed_images(b.handle))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            b(x[:n])
        assert int(N.lib().rva_yolov8_plan_primed_images(b.handle)) == before
        _fill(b.out)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(b.out[:n]), _bits(want)) and _untouched(b.out[n:])
    finally:
        b.concurrent_heads = lanes


# ---------------------------------------------------------------------------------------------------
# Detector
# ---------------------------------------------------------------------------------------------------
def _surface(rng, w, h):
    y, uv = rng.integers(16, 236, (h, w), dtype=np.uint8), rng.integers(16, 241, (h // 2, w), dtype=np.uint8)
    return ops.Nv12Surface.from_numpy(y, uv, w, h), (y, uv)


def test_detector_serves_every_live_count_from_one_plan(monkeypatch, caplog):
    """Case 9: detector A gets the live frames of a tick, detector B the same frames plus fillers up to the capacity."""
    monkeypatch.setenv("RVA_SKIP_VARIANTS", " ".join(str(v) for v in range(1, N.lib().rva_conv_num_variants() + 1)))
    monkeypatch.setenv("RVA_TUNE_CACHE", "0")
    monkeypatch.delenv("RVA_PLAN_NO_STATIC_ROWS", raising=False)
    net = build_detector_net("n", seed=0)
    cfg = dict(model_path="yolov8n.pt", backend="hip", half=True, confidence_threshold=0.25, warmup=False, hip_plan_capacity=4)
    A = HipYoloDetector(DetectorConfig(**cfg), net=copy.deepcopy(net))
    Bd = HipYoloDetector(DetectorConfig(**cfg), net=copy.deepcopy(net))
    assert A.plan_capacity == 4 and A.engine == "fused"
    calls = []                                             # (leading address of `out`, content_only) of every K1 launch
    real_k1 = ops.preprocess_nv12

    def k1_spy(*a, **kw):
        calls.append((kw["out"].data_ptr(), bool(kw.get("content_only", False))))
        return real_k1(*a, **kw)
    monkeypatch.setattr(ops, "preprocess_nv12", k1_spy)
    rng = np.random.default_rng(4)
    steady_a, steady_b = [], []
    state = {"A": (None, 0), "B": (None, 0)}               # the rule: steady = geometry unchanged and n within the images bordered so far

    def rule(who, geom, n):
        g, c = state[who]
        steady = g == geom and n <= c
        if not steady:
            state[who] = (geom, n)
        return steady
    for (w, h), counts in (((1920, 1080), (4, 4, 3, 4, 2, 1, 4)), ((1440, 1080), (3, 4))):
        for n in counts:
            made = [_surface(rng, w, h) for _ in range(4)]
            frames = [m[0] for m in made]
            A.predict_batch_device([SimpleNamespace(frame=f) for f in frames[:n]])
            Bd.predict_batch_device([SimpleNamespace(frame=f) for f in frames])
            torch.cuda.synchronize()
            assert list(A._plans) == [(4, 640, 640)] and list(Bd._plans) == [(4, 640, 640)] and list(A._in_bufs) == [4]
            pa, pb = A._plans[(4, 640, 640)], Bd._plans[(4, 640, 640)]
            assert torch.equal(_bits(pa.out[:n]), _bits(pb.out[:n])), ("head images [0, n)", (w, h), n)
            xin = A._in_bufs[4][:n].cpu().numpy().view(np.uint16)
            for j in range(n):
                want = orc.preprocess_nv12(made[j][1][0], made[j][1][1], w, h, 640, 640, True)[0].view(np.uint16)
                assert np.array_equal(xin[j], want), ("K1 input image", (w, h), n, j)
            (pa_ptr, got_a), (pb_ptr, got_b) = calls[-2], calls[-1]
            assert pa_ptr == A._in_bufs[4].data_ptr() and pb_ptr == Bd._in_bufs[4].data_ptr()
            steady_a.append(got_a)
            steady_b.append(got_b)
            assert got_a == rule("A", (w, h), n) and got_b == rule("B", (w, h), 4), ("content-only K1", (w, h), n)
    assert steady_a == [False, True, True, True, True, True, True, False, False], steady_a
    assert steady_b == [False, True, True, True, True, True, True, False, True], steady_b
    assert len(calls) == 18
    # a group larger than the capacity: an exact-size plan as without the key, and one warning
    with caplog.at_level(logging.WARNING, logger="realtime_video_analytics_32streams_amd.detector"):
        five = [_surface(rng, 1440, 1080)[0] for _ in range(5)]
        post = A.predict_batch_device([SimpleNamespace(frame=f) for f in five])
        A.predict_batch_device([SimpleNamespace(frame=f) for f in five])
        torch.cuda.synchronize()
    assert post is not None and list(A._plans) == [(4, 640, 640), (5, 640, 640)]
    assert sum("hip_plan_capacity" in r.getMessage() for r in caplog.records) == 1


# ---------------------------------------------------------------------------------------------------
# Pipeline
# ---------------------------------------------------------------------------------------------------
DROPS = {3: (2,), 4: (2,), 6: (0, 3)}                      # tick -> streams that deliver nothing


@pytest.mark.parametrize("mode", ["pipelined", "tick"])
def test_pipeline_with_streams_that_drop_frames(mode, monkeypatch):
    """Case 10: four 1080p streams, a calibrated YOLOv8n with capacity 4, ten ticks, each checked against the oracle: the input
    images are the oracle's K1 of what was delivered, every live stream's head image gives the oracle's track table, a stream that
    delivered nothing keeps its table, and the plans are the slots' -- none is added when the live count changes."""
    S, T = 4, 10
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    det = HipYoloDetector(DetectorConfig(model_path="yolov8n.pt", backend="hip", model_type="yolov8", warmup=False, half=True,
                                         confidence_threshold=0.25, hip_plan_capacity=S), net=build_detector_net("n", seed=0))
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs], (640, 640), half=True)
    calibrate_detection_density(det.net, sample.contiguous(memory_format=torch.channels_last), 0.25, 120)
    det.invalidate_engine()
    tcfg = TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1)
    trk = IouTracker(tcfg, max_streams=S, capacity=1024)
    pipe = TickPipeline(streams, det, trk, sources=srcs)
    runner = PipelinedTicks(pipe, depth=2, use_graph=True) if mode == "pipelined" else None
    otr = orc.Tracker(S, tcfg.max_age, tcfg.max_iou_distance, tcfg.min_hits)
    delivered = [[] for _ in range(S)]                     # per stream and tick: ring index of the delivered surface, or None
    for s, src in enumerate(srcs):
        def deliver(s=s, src=src, real=src.next_packet):
            p = real()
            k = len(delivered[s])
            if s in DROPS.get(k, ()):
                delivered[s].append(None)
                return None
            delivered[s].append(next(j for j, f in enumerate(src._ring) if f is p.frame))
            return p
        monkeypatch.setattr(src, "next_packet", deliver)
    want_k1, last = {}, [None] * S
    checked = 0

    def oracle_k1(s, j):
        if (s, j) not in want_k1:
            f = srcs[s]._ring[j]
            want_k1[(s, j)] = orc.preprocess_nv12(f.y.cpu().numpy(), f.uv.cpu().numpy(), 1920, 1080, 640, 640, True)[0].view(np.uint16)
        return want_k1[(s, j)]

    def check(k, tables, par):
        nonlocal checked
        live = [s for s in range(S) if delivered[s][k] is not None]
        n = len(live)
        assert n == S - len(DROPS.get(k, ()))
        x = det._in_bufs[S if par == 0 else (S, par)][:n].cpu().numpy().view(np.uint16)
        for j, s in enumerate(live):
            assert np.array_equal(x[j], oracle_k1(s, delivered[s][k])), ("K1 input tensor", k, s)
        head = det._plans[(S, 640, 640) if par == 0 else (S, 640, 640, par)]._outs[0][:n].float().cpu().numpy()
        for s in range(S):                                 # canonical order: tick-major, stream-minor
            if s in live:
                r = orc.postprocess(head[live.index(s)], det.config.confidence_threshold, det.config.iou_threshold, None, (1920, 1080))
                m = r["conf"].astype(np.float64) >= det.config.confidence_threshold
                last[s] = otr.update(s, r["boxes"][m].astype(np.float64), r["conf"][m].astype(np.float64), r["cls"][m].astype(np.int64))
                checked += last[s]["n"]
            assert last[s] is not None and orc.table_of(tables[s]) == orc.table_of(last[s]), (k, s, "live" if s in live else "no frame")
    plans_after = []
    if runner is not None:
        done = 0

        def collect():
            nonlocal done
            _, tables = runner.collect()
            check(done, tables, done % runner.nslots)
            done += 1
        for k in range(T):
            if k - done == runner.depth:
                collect()
            runner.submit()
            plans_after.append(len(det._plans))
        while done < T:
            collect()
        slots = runner.nslots
    else:
        for k in range(T):
            pipe.tick()
            plans_after.append(len(det._plans))
            check(k, trk.device_tracker.read_all(), 0)
        slots = 1
    assert plans_after[1:] == [slots] * (T - 1), plans_after       # one plan per slot in use, none added after the first two ticks
    assert all(key[0] == S for key in det._plans), list(det._plans)
    assert checked > 0
