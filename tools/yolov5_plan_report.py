"""Measurement report of the fused fp16 YOLOv5 plan -> profiles/yolov5_plan.json.

  * forward pass alone: YOLOv5s and YOLOv5n at 1 / 8 / 32 images, 640 x 640, the plan (autotuned) against the same fused module as
    PyTorch-ROCm fp16 channels-last; five alternated runs (the order turned round every time), median, all five and their spread;
  * per-step times of YOLOv5s x 32 (device events around 20 repetitions of every step of the plan), the stem and the three head
    steps among them, and ``rva_stem_conv_f16`` (``k_stem``, the 3x3 stem of YOLOv8) at the same output shape: it moves the same bytes;
  * 32 x 1920x1080 NV12 streams through ``PipelinedTicks`` at depth 1 and 4: frames/s, p50 / p99 tick latency;
  * accuracy: what tests/test_gpu_yolov5_prims.py and tests/test_gpu_yolov5_plan.py record (max observed / bound per row kind of the
    two kernels; the plan's and PyTorch fp16's largest error against the float64 module) -- the tool runs those tests with
    ``RVA_REPORT_DIR`` set and copies their records.

Every leg is a child process under its own ``timeout -k 10``; the driver touches no GPU and stops at the first child that fails.
GPU only: ``python tools/yolov5_plan_report.py [--out FILE] [--skip-pipeline]``."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HW, PASSES, WARM = (640, 640), 30, 8


def _ms(fn, passes=PASSES, warm=WARM):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(passes):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / passes


def leg_forward(scale, batch, rounds):
    import torch
    sys.path.insert(0, str(ROOT))
    from realtime_video_analytics_32streams_amd.engine import FusedYoloV5
    from realtime_video_analytics_32streams_amd.yolov5 import build_detector_net_v5
    net = build_detector_net_v5(scale, seed=0).fuse()
    x = torch.rand((batch, 3, *HW), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).half()
    plan = FusedYoloV5(net, batch, HW)
    ref = build_detector_net_v5(scale, seed=0).fuse().half().cuda().to(memory_format=torch.channels_last)
    xcl = x.contiguous(memory_format=torch.channels_last)

    def run_torch():
        with torch.inference_mode():
            ref(xcl)
    a, b = [], []
    for i in range(rounds):
        legs = [lambda: a.append(_ms(lambda: plan(x))), lambda: b.append(_ms(run_torch))]
        for leg in (legs if i % 2 else legs[::-1]):
            leg()
    print("LEG " + json.dumps({"plan_ms": a, "torch_fp16_ms": b, "launches": plan.n_launches,
                               "selection": [[d, int(st["variant"])] for _, st, d in plan._tunable]}))


def leg_steps(scale, batch):
    import torch
    sys.path.insert(0, str(ROOT))
    from realtime_video_analytics_32streams_amd import _native as N
    from realtime_video_analytics_32streams_amd.engine import FusedYoloV5
    from realtime_video_analytics_32streams_amd.yolov5 import build_detector_net_v5
    net = build_detector_net_v5(scale, seed=0).fuse()
    x = torch.rand((batch, 3, *HW), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).half()
    plan = FusedYoloV5(net, batch, HW)
    plan(x)
    L, st = plan.L, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xin, out = C.c_void_p(x.data_ptr()), C.c_void_p(plan.out.data_ptr())
    c5 = net.b7.conv.out_channels
    descs = [d for _, _, d in plan._tunable]
    pool_after = descs.index(f"{c5}->{c5 // 2} k1s1 {HW[0] // 32}x{HW[1] // 32}")       # b9.cv1; the SPPF pools follow it
    names, t = ["stem6 (rva_stem6_conv_f16)"], 0
    while len(names) < plan._n_steps:
        names.append(descs[t]); t += 1
        if t == pool_after + 1:
            names.append("sppf pool3")
    rows = []
    for i, name in enumerate(names):
        ms = _ms(lambda: plan.ctx.check(L.rva_yolov8_plan_run_range_n(plan.handle, xin, out, batch, i, i + 1, st), "run_range"), 20, 3)
        rows.append({"step": i, "what": name, "us": round(ms * 1e3, 2)})
    # k_stem (the 3x3 stem) at the same output shape
    c1 = net.b0.conv.out_channels
    y = torch.empty((batch, HW[0] // 2, HW[1] // 2, c1), dtype=torch.float16, device="cuda")
    w3 = torch.zeros((64, 32), dtype=torch.float16, device="cuda").normal_(0, 0.1)
    b3 = torch.zeros(64, dtype=torch.float32, device="cuda")
    ms3 = _ms(lambda: plan.ctx.check(L.rva_stem_conv_f16(plan.ctx.handle, xin, C.c_void_p(w3.data_ptr()), C.c_void_p(b3.data_ptr()),
                                                         C.c_void_p(y.data_ptr()), c1, batch, HW[0], HW[1], c1, st), "rva_stem_conv_f16"), 20, 3)
    print("LEG " + json.dumps({"scale": scale, "batch": batch, "us_sum": round(sum(r["us"] for r in rows), 1), "steps": rows,
                               "k_stem_3x3_same_output_shape_us": round(ms3 * 1e3, 2), "stem_cout": c1}))


def leg_pipeline(depth, ticks=100, warm=20):
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
    from realtime_video_analytics_32streams_amd.detector import create_detector
    from realtime_video_analytics_32streams_amd import ops
    from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
    from realtime_video_analytics_32streams_amd.tracker import IouTracker
    from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream
    from realtime_video_analytics_32streams_amd.yolov5 import calibrate_detection_density_v5
    S = 32
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", target_fps=30.0, warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    det = create_detector(DetectorConfig(backend="hip", model_type="yolov5", model_path="yolov5s.pt", half=True, warmup=False,
                                         confidence_threshold=0.25))
    det.tune_overlap = depth
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs[:8]], HW, half=True)
        calibrate_detection_density_v5(det.net, sample.clone().contiguous(memory_format=torch.channels_last), 0.25, 120)
    det.invalidate_engine()
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=S, capacity=1024)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth)
    for _ in range(warm):
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    lat, t_enq, done = [], {}, 0
    t0 = time.perf_counter()
    for k in range(ticks):
        if k - done == runner.depth:
            runner.collect(); lat.append(time.perf_counter() - t_enq[done]); done += 1
        t_enq[k] = time.perf_counter()
        runner.submit()
    while done < ticks:
        runner.collect(); lat.append(time.perf_counter() - t_enq[done]); done += 1
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    print("LEG " + json.dumps({"engine": det.engine, "arch": det.arch, "depth": runner.depth, "streams": S, "ticks": ticks,
                               "frames_per_s": ticks * S / el, "p50_tick_ms": float(np.percentile(lat, 50) * 1e3),
                               "p99_tick_ms": float(np.percentile(lat, 99) * 1e3)}))


def child(args, env, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, *args], capture_output=True, text=True, env=env, cwd=str(ROOT))
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-3000:] + p.stderr[-4000:])
        raise SystemExit(f"yolov5_plan_report: child {args[:6]} ended with status {p.returncode}; stopping")
    return p.stdout


def leg(env, limit, *args):
    txt = child([str(Path(__file__).resolve()), *args], env, limit)
    return json.loads(next(line for line in txt.splitlines() if line.startswith("LEG "))[4:])


def summary(vals):
    import numpy as np
    return {"ms": round(float(np.median(vals)), 4), "ms_all": [round(v, 4) for v in vals], "spread_ms": round(max(vals) - min(vals), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--scale", default="s")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-tests", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "yolov5_plan.json"))
    a = ap.parse_args()
    if a.leg == "forward":
        return leg_forward(a.scale, a.batch, a.rounds)
    if a.leg == "steps":
        return leg_steps(a.scale, a.batch)
    if a.leg == "pipeline":
        return leg_pipeline(a.depth)
    rep = {"what": f"fused fp16 YOLOv5 plan at {HW[0]} x {HW[1]}; forward pass alone in ms per pass over {PASSES} passes, medians of "
                   f"{a.rounds} alternated runs against the same fused module as PyTorch-ROCm fp16 channels-last", "device": None,
           "forward": {}, "steps": None, "pipeline_32x1080p": {}, "accuracy": {}}
    out = Path(a.out)

    def save():
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rep, indent=1) + "\n")
    with tempfile.TemporaryDirectory() as cache, tempfile.TemporaryDirectory() as rdir:
        env = dict(os.environ, RVA_TUNE_CACHE_DIR=cache)
        rep["device"] = child(["-c", "import torch; print(torch.cuda.get_device_name(0))"], env, 120).strip().splitlines()[-1]
        for scale in ("s", "n"):
            for batch in (1, 8, 32):
                r = leg(env, 420, "--leg", "forward", "--scale", scale, "--batch", str(batch), "--rounds", str(a.rounds))
                p, t = summary(r["plan_ms"]), summary(r["torch_fp16_ms"])
                rep["forward"][f"yolov5{scale} x {batch}"] = {"plan": p, "torch_fp16": t, "plan_over_torch": round(p["ms"] / t["ms"], 3),
                                                              "launches": r["launches"], "selection": r["selection"]}
                save()
        rep["steps"] = leg(env, 420, "--leg", "steps", "--scale", "s", "--batch", "32")
        save()
        if not a.skip_pipeline:
            for depth in (1, 4):
                rep["pipeline_32x1080p"][f"depth {depth}"] = leg(env, 480, "--leg", "pipeline", "--depth", str(depth))
                save()
        if not a.skip_tests:
            tenv = dict(env, RVA_REPORT_DIR=rdir)
            child(["-m", "pytest", "-q", "-m", "gpu", "tests/test_gpu_yolov5_prims.py", "tests/test_gpu_yolov5_plan.py"], tenv, 480)
            for name, key in (("yolov5_bounds.json", "kernels_max_observed_over_bound"), ("yolov5_accuracy.json", "plan_against_float64_module")):
                f = Path(rdir) / name
                rep["accuracy"][key] = json.loads(f.read_text()) if f.exists() else "not recorded"
        save()
    print(json.dumps(rep, indent=1))


if __name__ == "__main__":
    main()
