"""Measurement report of the fused fp16 YOLO11 plan -> profiles/yolo11_plan.json.

  * forward pass alone: YOLO11n and YOLO11s at 1 / 8 / 32 images, 640 x 640, the plan (autotuned) against the same fused module as
    PyTorch-ROCm fp16 channels-last; five alternated runs (the order turned round every time), median, all five and their spread;
  * per-step times of YOLO11n x 32 (device events around 20 repetitions of every step of the plan, named by
    ``rva_yolov8_plan_step_desc``).  The attention and depthwise steps carry the bytes and FLOPs the algorithm needs, computed from
    their shapes, and the least time the hardware could take for them: the larger of bytes / 8.0 TB/s (HBM3E peak) and FLOPs over
    the peak rate (2.5 PFLOP/s fp16 MFMA for attention, 157.3 TFLOP/s fp32 vector for the depthwise steps), and which of the two
    bounds it;
  * 32 x 1920x1080 NV12 streams through ``PipelinedTicks`` at depth 1 and 4: frames/s, p50 / p99 tick latency;
  * accuracy: what tests/test_gpu_yolo11_plan.py records (the plan's and PyTorch fp16's largest error against the float64 module) --
    the tool runs that file with ``RVA_REPORT_DIR`` set and copies its record.

Every leg is a child process under its own ``timeout -k 10``; the driver touches no GPU and stops at the first child that fails.  A
leg that was skipped is reported as "not measured".
GPU only: ``python tools/yolo11_plan_report.py [--out FILE] [--only forward|steps|pipeline|tests ...]``."""
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
SECTIONS = ("forward", "steps", "pipeline", "tests")
HBM_BYTES_PER_S, MFMA_F16_FLOPS, VALU_F32_FLOPS = 8.0e12, 2.5e15, 157.3e12


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
    from realtime_video_analytics_32streams_amd.engine import FusedYolo11
    from realtime_video_analytics_32streams_amd.yolo11 import build_detector_net_11
    net = build_detector_net_11(scale, seed=0).fuse()
    x = torch.rand((batch, 3, *HW), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).half()
    plan = FusedYolo11(net, batch, HW)
    ref = build_detector_net_11(scale, seed=0).fuse().half().cuda().to(memory_format=torch.channels_last)
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


def step_roofline(desc, batch, psa_width):
    """Bytes and FLOPs of an attention or depthwise step from its description, and the least time the hardware could take."""
    f = desc.split()
    if f[0] == "attention":
        heads, tokens = int(f[2]), int(f[4])
        nbytes = batch * tokens * (2 * psa_width + psa_width) * 2            # qkv read once, the heads' outputs written
        flops = batch * heads * 2 * tokens * tokens * (32 + 64)              # S = Q K^T (32) and O = P V (64)
        t_flop = flops / MFMA_F16_FLOPS
    elif f[0] == "dwconv3x3":
        c = int(f[1])
        h, w = (int(v) for v in f[-1].split("x"))
        nbytes = batch * h * w * c * 2 * (3 if "+res" in f else 2)           # input, output, residual
        flops = batch * h * w * c * 18
        t_flop = flops / VALU_F32_FLOPS
    else:
        return None
    t_mem = nbytes / HBM_BYTES_PER_S
    return {"bytes": nbytes, "flops": flops, "floor_us": round(max(t_mem, t_flop) * 1e6, 3), "bound_by": "bytes" if t_mem >= t_flop else "flops"}


def step_kind(desc):
    """The row of the by-kind table a step belongs to."""
    first = desc.split()[0]
    if first in ("attention", "dwconv3x3", "stem", "stem2", "sppf", "head3"):
        return first
    if desc.startswith("head"):
        return "head 1x1 + decode"
    if desc.startswith("up"):
        return "upsample + concat 1x1"
    return "conv " + desc.split()[1]                      # "64->128 k3s2 80x80" -> "conv k3s2"


def leg_steps(scale, batch):
    import torch
    sys.path.insert(0, str(ROOT))
    from realtime_video_analytics_32streams_amd.engine import FusedYolo11
    from realtime_video_analytics_32streams_amd.yolo11 import build_detector_net_11
    net = build_detector_net_11(scale, seed=0).fuse()
    x = torch.rand((batch, 3, *HW), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).half()
    plan = FusedYolo11(net, batch, HW)
    plan(x)
    L, st = plan.L, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xin, out = C.c_void_p(x.data_ptr()), C.c_void_p(plan.out.data_ptr())
    rows = []
    for i in range(plan.n_launches):
        ms = _ms(lambda: plan.ctx.check(L.rva_yolov8_plan_run_range_n(plan.handle, xin, out, batch, i, i + 1, st), "run_range"), 20, 3)
        row = {"step": i, "what": plan.step_desc(i), "us": round(ms * 1e3, 2)}
        roof = step_roofline(row["what"], batch, net.l10.c)
        if roof:
            row.update(roof, share_of_floor=round(roof["floor_us"] / max(row["us"], 1e-9), 4))
        rows.append(row)
    total = sum(r["us"] for r in rows)
    kinds = {}
    for r in rows:
        kinds[step_kind(r["what"])] = round(kinds.get(step_kind(r["what"]), 0.0) + r["us"], 2)
    print("LEG " + json.dumps({"scale": scale, "batch": batch, "us_sum": round(total, 1), "us_by_kind": dict(sorted(kinds.items(), key=lambda kv: -kv[1])),
                               "steps": rows}))


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
    from realtime_video_analytics_32streams_amd.yolo11 import calibrate_detection_density_11
    S = 32
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", target_fps=30.0, warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    det = create_detector(DetectorConfig(backend="hip", model_path="yolo11n.pt", half=True, warmup=False, confidence_threshold=0.25))
    det.tune_overlap = depth
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs[:8]], HW, half=True)
        calibrate_detection_density_11(det.net, sample.clone().contiguous(memory_format=torch.channels_last), 0.25, 120)
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
    print("LEG " + json.dumps({"engine": det.engine, "arch": det.arch, "model": "yolo11n", "depth": runner.depth, "streams": S, "ticks": ticks,
                               "frames_per_s": ticks * S / el, "p50_tick_ms": float(np.percentile(lat, 50) * 1e3),
                               "p99_tick_ms": float(np.percentile(lat, 99) * 1e3)}))


def child(args, env, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, *args], capture_output=True, text=True, env=env, cwd=str(ROOT))
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-3000:] + p.stderr[-4000:])
        raise SystemExit(f"yolo11_plan_report: child {args[:6]} ended with status {p.returncode}; stopping")
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
    ap.add_argument("--scale", default="n")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", action="append", choices=SECTIONS,
                    help="measure these sections only (repeatable) and keep the others as the file at --out has them")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "yolo11_plan.json"))
    a = ap.parse_args()
    if a.leg == "forward":
        return leg_forward(a.scale, a.batch, a.rounds)
    if a.leg == "steps":
        return leg_steps(a.scale, a.batch)
    if a.leg == "pipeline":
        return leg_pipeline(a.depth)
    rep = {"what": f"fused fp16 YOLO11 plan at {HW[0]} x {HW[1]}; forward pass alone in ms per pass over {PASSES} passes, medians of "
                   f"{a.rounds} alternated runs against the same fused module as PyTorch-ROCm fp16 channels-last", "device": None,
           "forward": {}, "steps": "not measured", "pipeline_32x1080p": "not measured", "accuracy": "not measured"}
    out = Path(a.out)
    todo = a.only or list(SECTIONS)
    if a.only and out.exists():
        rep.update(json.loads(out.read_text()))

    def save():
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rep, indent=1) + "\n")
    with tempfile.TemporaryDirectory() as cache, tempfile.TemporaryDirectory() as rdir:
        env = dict(os.environ, RVA_TUNE_CACHE_DIR=cache)
        rep["device"] = child(["-c", "import torch; print(torch.cuda.get_device_name(0))"], env, 120).strip().splitlines()[-1]
        for scale in ("n", "s") if "forward" in todo else ():
            for batch in (1, 8, 32):
                r = leg(env, 420, "--leg", "forward", "--scale", scale, "--batch", str(batch), "--rounds", str(a.rounds))
                p, t = summary(r["plan_ms"]), summary(r["torch_fp16_ms"])
                rep["forward"][f"yolo11{scale} x {batch}"] = {"plan": p, "torch_fp16": t, "plan_over_torch": round(p["ms"] / t["ms"], 3),
                                                              "launches": r["launches"], "selection": r["selection"]}
                save()
        if "steps" in todo:
            rep["steps"] = leg(env, 420, "--leg", "steps", "--scale", "n", "--batch", "32")
            save()
        if "pipeline" in todo:
            rep["pipeline_32x1080p"] = {}
            for depth in (1, 4):
                rep["pipeline_32x1080p"][f"depth {depth}"] = leg(env, 480, "--leg", "pipeline", "--depth", str(depth))
                save()
        if "tests" in todo:
            child(["-m", "pytest", "-q", "-m", "gpu", "tests/test_gpu_yolo11_plan.py"], dict(env, RVA_REPORT_DIR=rdir), 480)
            f = Path(rdir) / "yolo11_accuracy.json"
            rep["accuracy"] = {"plan_against_float64_module": json.loads(f.read_text()) if f.exists() else "not recorded"}
        save()
    print(json.dumps(rep, indent=1))


if __name__ == "__main__":
    main()
