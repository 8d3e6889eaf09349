"""Measurement report of ``hip_plan_capacity`` (one YOLOv8 plan that serves every live-stream count) -> profiles/plan_capacity.json.

32 x 1080p YOLOv8s fp16 through ``PipelinedTicks`` at the default depth, twice in ONE process on one box: with
``hip_plan_capacity: 0`` (a plan per batch size: the behaviour before the key existed, the yardstick) and with ``32``.  Recorded:

  * ``first_tick_ms``: wall time (submit -> collect) of the first tick at each new live count, 31 down to 24 streams;
  * ``device_memory``: bytes in use on the device before and after that sweep;
  * ``workspace_bytes``: what one 32-image plan takes (device memory in use after against before its construction);
  * ``frames_per_s``: the full count both ways, five alternated runs, medians and spread;
  * ``forward_n24_us``: the forward pass of 24 images on the capacity-32 plan against an exact 24-image plan.

None of these is a gate.  The run at 0 is the yardstick, and a difference counts only beyond that run's own spread.
Run it under a time limit of the caller's; any error ends the process.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")             # as bench.py: the tick chains on queues of their own
S = 32


def used_bytes():
    import torch
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return int(total - free)


def make_runner(capacity):
    import torch

    from realtime_video_analytics_32streams_amd import ops
    from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
    from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
    from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
    from realtime_video_analytics_32streams_amd.tracker import IouTracker
    from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    det = HipYoloDetector(DetectorConfig(model_path="yolov8s.pt", backend="hip", half=True, warmup=False, confidence_threshold=0.25,
                                         hip_plan_capacity=capacity), net=build_detector_net("s", seed=0))
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs[:8]], (640, 640), half=True)
        calibrate_detection_density(det.net, sample.contiguous(memory_format=torch.channels_last), 0.25, 120)
    det.invalidate_engine()
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=S, capacity=1024)
    return PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), use_graph=True), det, srcs


def drain(runner):
    while runner._oldest < runner._next:
        runner.collect()


def throughput(runner, seconds):
    import torch
    drain(runner)
    for _ in range(2 * runner.depth):                      # back on the full count: the captured shape
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    done = k = 0
    t0 = time.perf_counter()
    while True:
        if k - done == runner.depth:
            runner.collect(); done += 1
        runner.submit(); k += 1
        if time.perf_counter() - t0 > seconds and k >= 30:
            break
    while done < k:
        runner.collect(); done += 1
    return round(S * k / (time.perf_counter() - t0), 1)


def sweep(runner, det, srcs):
    """One tick alone at each live count 31 .. 24 (the streams behind the count deliver nothing): submit -> collect."""
    import torch
    drain(runner)
    out = {}
    before = used_bytes()
    plans_before = len(det._plans)
    for live in range(31, 23, -1):
        packets = [src.next_packet() if i < live else None for i, src in enumerate(srcs)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.submit(packets)
        runner.collect()
        out[str(live)] = round((time.perf_counter() - t0) * 1e3, 2)
    after = used_bytes()
    return {"first_tick_ms": out, "device_memory": {"before_bytes": before, "after_bytes": after, "grown_bytes": after - before},
            "plans": {"before": plans_before, "after": len(det._plans)}}


def forward_us(plan, x, reps=30):
    import torch
    for _ in range(3):
        plan(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            plan(x)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return round(best, 1)


def spread_pct(vals):
    return round((max(vals) - min(vals)) / (sum(vals) / len(vals)) * 100, 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="short windows (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_capacity.json"))
    args = ap.parse_args()
    os.environ.setdefault("RVA_TUNE_CACHE_DIR", tempfile.mkdtemp(prefix="plan_capacity_tune_"))       # both ways start without a selection
    import torch

    from realtime_video_analytics_32streams_amd.engine import FusedYoloV8
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net
    torch.cuda.set_device(0)
    out = {"what": __doc__.split("\n")[0], "device": torch.cuda.get_device_name(0), "streams": S}
    sec = 1.0 if args.quick else 3.0

    # what one plan takes
    net = build_detector_net("s", seed=0)
    m0 = used_bytes()
    probe = FusedYoloV8(net, S, autotune=False)
    out["workspace_bytes"] = used_bytes() - m0
    del probe

    runners = {}
    for cap in (0, S):                                     # 0 first: it tunes the 32-image plan, 32 takes the selection from the cache
        t0 = time.perf_counter()
        runner, det, srcs = make_runner(cap)
        for _ in range(16):
            runner.submit(); runner.collect()
        torch.cuda.synchronize()
        assert runner._captured and det.plan_capacity == cap
        runners[cap] = (runner, det, srcs)
        out[f"capacity_{cap}"] = {"depth": runner.depth, "setup_and_16_ticks_s": round(time.perf_counter() - t0, 2),
                                  "kernel_selection": getattr(next(iter(det._plans.values())), "tuning_source", "?")}
    fps = {0: [], S: []}
    for _ in range(5):                                     # alternated on one box
        for cap in (0, S):
            fps[cap].append(throughput(runners[cap][0], sec))
    base = statistics.median(fps[0])
    out["frames_per_s"] = {f"capacity_{cap}": {"runs": v, "median": statistics.median(v), "spread_pct": spread_pct(v)} for cap, v in fps.items()}
    delta = round((statistics.median(fps[S]) / base - 1) * 100, 2)
    out["frames_per_s"]["capacity_32_against_0_pct"] = delta
    out["frames_per_s"]["beyond_the_spread_of_the_runs_at_0"] = bool(abs(delta) > spread_pct(fps[0]))
    for cap in (0, S):
        out[f"capacity_{cap}"].update(sweep(*runners[cap]))
    # the forward pass of 24 images: on the capacity plan (tuned at 32) and on a plan of exactly 24 (tuned at 24)
    x = torch.rand((S, 3, 640, 640), device="cuda").half()
    p32, p24 = FusedYoloV8(net, S), FusedYoloV8(net, 24)
    out["forward_n24_us"] = {"capacity_32_plan": forward_us(p32, x[:24]), "exact_24_plan": forward_us(p24, x[:24]),
                             "capacity_32_plan_full": forward_us(p32, x)}
    out["forward_n24_us"]["capacity_against_exact_pct"] = round(
        (out["forward_n24_us"]["capacity_32_plan"] / out["forward_n24_us"]["exact_24_plan"] - 1) * 100, 2)
    p = Path(args.out)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    print("wrote", p)


if __name__ == "__main__":
    main()
