"""Batched previews against one ``render_frame`` per stream, on the GPU box -> profiles/preview_batch.json.

Part 1: for B = 1, 8, 32 previews of 1920x1080 surfaces, and 8 of 3840x2160 (-> 1080p), the wall time and the device time
(HIP events around the whole call) of B sequential ``preview.render_frame`` calls and of one ``preview.render_frames`` call --
five alternated runs, medians and spread (max - min); the data URLs of the two paths are asserted equal.  Clocks are left alone.
Part 2: one ``PipelinedTicks`` leg (32 x 1080p, YOLOv8s, default depth) with a scripted policy clock that makes every third tick
a preview tick: frames/s and per-tick wall time (submit .. collect_result), p99 over all ticks and over the preview ticks, with
``previews`` unset and set.
Usage: python tools/preview_batch_report.py [--out profiles/preview_batch.json] [--ticks 150] [--skip-pipeline]"""
import argparse
import copy
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from realtime_video_analytics_32streams_amd import ops, synth  # noqa: E402
from realtime_video_analytics_32streams_amd import preview as P  # noqa: E402

RUNS = 5


def tracks_for(n, w, h, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        bw, bh = int(rng.integers(w // 10, w // 4)), int(rng.integers(h // 10, h // 4))
        x0, y0 = float(rng.integers(0, w - bw)), float(rng.integers(0, h - bh))
        out.append({"track_id": 17 * k + seed, "class_id": int(rng.integers(0, 80)), "confidence": 0.6,
                    "bbox_xyxy": [x0 + 0.5, y0 + 0.5, x0 + bw, y0 + bh]})
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
            "spread_ms": round(max(v) - min(v), 3)}


def previews_part(rows):
    pol = P.PreviewPolicy(frame_quality=75)
    for (w, h, B) in ((1920, 1080, 1), (1920, 1080, 8), (1920, 1080, 32), (3840, 2160, 8)):
        pitch = ((w + 255) // 256) * 256
        uniq = [synth.make_nv12(100 + i, w, h, pitch) for i in range(min(B, 4))]      # four distinct pictures, B surfaces of their own
        surfs = [ops.Nv12Surface.from_numpy(*uniq[i % len(uniq)], w, h) for i in range(B)]
        tracks = [tracks_for((3 * i) % 12, w, h, i) for i in range(B)]
        qs = [pol.adaptive_quality(len(t)) for t in tracks]
        batcher = P.PreviewBatcher(pol, max_streams=B)
        seq = lambda: [P.render_frame(s, t, q, pol) for s, t, q in zip(surfs, tracks, qs)]      # noqa: E731
        bat = lambda: batcher.render(surfs, tracks, qs)                                          # noqa: E731
        a, b = seq(), bat()                                                                      # warm-up; and the contract
        assert a == b, f"render_frames differs from render_frame at {w}x{h} B={B}"
        seq(); bat()
        t = {"seq_wall": [], "seq_dev": [], "bat_wall": [], "bat_dev": []}
        for _ in range(RUNS):                                                                   # alternated
            ra, wa, da = timed(seq)
            rb, wb, db = timed(bat)
            assert ra == rb == a
            t["seq_wall"].append(wa); t["seq_dev"].append(da); t["bat_wall"].append(wb); t["bat_dev"].append(db)
        row = {"surface": [w, h], "previews": B, "jpeg_bytes_total": sum(len(u) for u in a) * 3 // 4,
               "sequential_render_frame": {"wall": stats(t["seq_wall"]), "device_span": stats(t["seq_dev"])},
               "one_render_frames": {"wall": stats(t["bat_wall"]), "device_span": stats(t["bat_dev"])},
               "wall_ratio_seq_over_batch": round(statistics.median(t["seq_wall"]) / statistics.median(t["bat_wall"]), 2),
               "faster_by_more_than_the_spread": statistics.median(t["seq_wall"]) - statistics.median(t["bat_wall"]) >
               max(stats(t["seq_wall"])["spread_ms"], stats(t["bat_wall"])["spread_ms"])}
        print(json.dumps(row), flush=True)
        rows.append(row)
        batcher.encoder.close()
        del batcher, surfs


def pipeline_leg(ticks, with_previews):
    from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
    from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
    from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
    from realtime_video_analytics_32streams_amd.tracker import IouTracker
    from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density
    S = 32
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", target_fps=30.0, warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=2, ring_frames=8) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    det = HipYoloDetector(DetectorConfig(model_path="yolov8s.pt", backend="hip", model_type="yolov8", half=True, confidence_threshold=0.25,
                                         warmup=False), net=copy.deepcopy(build_detector_net("s", seed=0)))
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs[:8]], (640, 640), half=True)
        calibrate_detection_density(det.net, sample.contiguous(memory_format=torch.channels_last), 0.25, 120)
    det.invalidate_engine()
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=S, capacity=1024)
    pipe = TickPipeline(streams, det, trk, sources=srcs)
    now = [1000.0]
    if with_previews:
        pipe.previews = P.PreviewBatcher(P.PreviewPolicy(frame_quality=75, clock=lambda: now[0]), max_streams=S)
    runner = PipelinedTicks(pipe)
    for _ in range(24):                                              # plan tuning, graph capture, clocks
        now[0] += 1.0 / 30
        runner.submit(); runner.collect_result()
    torch.cuda.synchronize()
    wall = np.empty(ticks)
    is_prev = np.zeros(ticks, bool)
    t_enq, done = {}, 0
    t_all = time.perf_counter()

    def collect():
        nonlocal done
        now[0] = 2000.0 + done * 0.0334                             # the policy clock follows the stream's frame time: every third tick is due
        r = runner.collect_result()
        wall[done] = time.perf_counter() - t_enq[done]
        is_prev[done] = bool(r.frame_jpeg)
        done += 1
    for k in range(ticks):
        if k - done == runner.depth:
            collect()
        t_enq[k] = time.perf_counter()
        runner.submit()
    while done < ticks:
        collect()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_all
    p = lambda v, q: round(float(np.percentile(v, q)) * 1e3, 3) if len(v) else None      # noqa: E731
    return {"previews": "set" if with_previews else "unset", "ticks": ticks, "ticks_in_flight": runner.depth,
            "frames_per_s": round(S * ticks / elapsed, 1), "tick_ms_p50": p(wall, 50), "tick_ms_p99": p(wall, 99),
            "preview_ticks": int(is_prev.sum()), "preview_tick_ms_p50": p(wall[is_prev], 50), "preview_tick_ms_p99": p(wall[is_prev], 99),
            "every_third_tick_ms_p99": p(wall[0::3], 99)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--ticks", type=int, default=150)
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    rep = {"device": torch.cuda.get_device_name(0), "protocol": f"{RUNS} alternated runs per path after two warm-up runs; wall = host time "
           "around the whole call(s) incl. the final synchronisation, device_span = HIP events around the same; clocks left alone",
           "previews": [], "pipeline": []}
    previews_part(rep["previews"])
    if args.out:
        Path(args.out).write_text(json.dumps(rep, indent=1))
    if not args.skip_pipeline:
        for with_previews in (False, True):
            leg = pipeline_leg(args.ticks, with_previews)
            print(json.dumps(leg), flush=True)
            rep["pipeline"].append(leg)
            if args.out:
                Path(args.out).write_text(json.dumps(rep, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
