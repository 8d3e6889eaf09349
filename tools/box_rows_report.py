"""Measurement report of the fp32 box rows of the fp16 plan (``hip_box_rows: fp32``) -> profiles/box_rows_f32.json.

On class-bias-calibrated weights (scores around 0.25, as ``_calibrated_error_report`` of tests/test_gpu_engine.py sets them up), for
n x 2, m x 4 and s x 32:
  * ``box_px`` max / mean / p99.9 of ``boxes32`` and of the fp16 rows of the same run, each against the plain fp32 module and
    against the rounding-matched reference (tests/helpers.py::plan_rounded_reference);
  * how much of what remains against the fp32 module is the fp16 rounding of the box LOGITS: the rounding-matched reference
    evaluated in torch once with and once without that one rounding (what taking the DFL from the unrounded accumulators could
    remove; not built);
  * threshold flips at 0.25 in both modes (equal: the class rows are the same bits).
Speed, a record and not a gate (the mode is opt-in): 32 x 1080p NV12, YOLOv8s through PipelinedTicks at depth 1 and 4 with the
option off and on, alternated, two runs each (frames/s, p99 tick latency), and the K2 / head-launch times of one
``rocprofv3 --kernel-trace --stats`` run per mode.

The driver (no ``--leg``) touches no GPU itself: it runs every leg as a child process under its own ``timeout -k 10`` and stops at
the first leg that fails.  All legs share one kernel-selection cache of their own (``RVA_TUNE_CACHE_DIR``): the first leg of a plan
shape times the variants, the others -- both modes, the cache key is the same -- run the same selection, and the profiled runs
contain no tuning launches.  GPU only: ``python tools/box_rows_report.py [--quick] [--out FILE]``.
"""
from __future__ import annotations

import argparse
import copy
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SIZES = (("n", 2), ("m", 4), ("s", 32))


# ------------------------------------------------------------------------------------------------ accuracy leg (child)
def matched_reference(net, x, round_box_logits=True):
    """tests/helpers.py::plan_rounded_reference with ONE switch: whether the last 1x1 convolution of the box branch is rounded
    to fp16 logits (what the plan does) or feeds the DFL unrounded.  Everything else rounds where the plan rounds."""
    import torch
    import torch.nn.functional as F

    from realtime_video_analytics_32streams_amd.yolov8 import ConvBnAct
    net = copy.deepcopy(net).fuse().float().to(x.device)
    r16 = lambda t: t.half().float()                                        # noqa: E731

    def cba(m, t, rnd=True):
        conv = m.conv if isinstance(m, ConvBnAct) else m
        y = F.conv2d(t, r16(conv.weight), conv.bias.float(), conv.stride, conv.padding)
        if isinstance(m, ConvBnAct) and m.act:
            y = F.silu(y)
        return r16(y) if rnd else y

    def c2f(m, t):
        y = list(cba(m.cv1, t).chunk(2, 1))
        for b in m.m:
            z = cba(b.cv2, cba(b.cv1, y[-1]))
            y.append(r16(y[-1] + z) if b.add else z)
        return cba(m.cv2, torch.cat(y, 1))

    def sppf(m, t):
        y = [cba(m.cv1, t)]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], m.k, 1, m.k // 2))
        return cba(m.cv2, torch.cat(y, 1))

    up = lambda t: F.interpolate(t, scale_factor=2.0, mode="nearest")        # noqa: E731
    dev = x.device
    with torch.inference_mode():
        t = x.half().float()
        t = c2f(net.b2, cba(net.b1, cba(net.b0, t)))
        p3 = c2f(net.b4, cba(net.b3, t))
        p4 = c2f(net.b6, cba(net.b5, p3))
        p5 = sppf(net.b9, c2f(net.b8, cba(net.b7, p4)))
        n4 = c2f(net.h12, torch.cat((up(p5), p4), 1))
        n3 = c2f(net.h15, torch.cat((up(n4), p3), 1))
        m4 = c2f(net.h18, torch.cat((cba(net.h16, n3), n4), 1))
        m5 = c2f(net.h21, torch.cat((cba(net.h19, m4), p5), 1))
        outs = []
        for lvl, (f, stride) in enumerate(((n3, 8.0), (m4, 16.0), (m5, 32.0))):
            B, _, h, w = f.shape
            box, cls = net.detect.box[lvl], net.detect.cls[lvl]
            bl = cba(box[2], cba(box[1], cba(box[0], f)), rnd=round_box_logits).reshape(B, 4, 16, h * w)
            cl = cba(cls[2], cba(cls[1], cba(cls[0], f))).reshape(B, net.nc, h * w)
            e = torch.exp(bl - bl.max(2, keepdim=True).values)
            d = (e * torch.arange(16, device=dev, dtype=torch.float32).view(1, 1, 16, 1)).sum(2) / e.sum(2)
            ay, ax = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32) + 0.5,
                                    torch.arange(w, device=dev, dtype=torch.float32) + 0.5, indexing="ij")
            ax, ay = ax.reshape(1, -1), ay.reshape(1, -1)
            x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
            xywh = torch.stack(((x1 + x2) * 0.5 * stride, (y1 + y2) * 0.5 * stride, (x2 - x1) * stride, (y2 - y1) * stride), 1)
            outs.append(torch.cat((xywh, torch.sigmoid(cl)), 1))
        return torch.cat(outs, 2)


def _stats(err):
    e = err.abs().flatten()
    k = max(int(e.numel() * 0.999), 1)
    return {"max": float(e.max()), "mean": float(e.mean()), "p99_9": float(e.kthvalue(k).values)}


def leg_accuracy(scale, batch):
    import torch

    from realtime_video_analytics_32streams_amd.engine import FusedYoloV8
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density
    from tests.helpers import plan_rounded_reference
    torch.cuda.set_device(0)
    net = build_detector_net(scale, seed=0)
    x = torch.rand((batch, 3, 640, 640), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).half()
    cal = copy.deepcopy(net).fuse().float().cuda()
    chunks = range(0, batch, 8)
    with torch.inference_mode():
        calibrate_detection_density(cal, x[:min(batch, 4)].float(), 0.25, 120)
        want = torch.cat([cal(x[i:i + 8].float()) for i in chunks])
        p16 = FusedYoloV8(copy.deepcopy(cal), batch)
        p32 = FusedYoloV8(copy.deepcopy(cal), batch, autotune=False, box_rows="fp32")
        p32.copy_tuning(p16)
        h16 = p16(x).clone()
        h32 = p32(x)
        b32 = p32.boxes32
        matched = torch.cat([plan_rounded_reference(cal, x[i:i + 8]) for i in chunks])
        mine = torch.cat([matched_reference(cal, x[i:i + 8], True) for i in chunks])
        unrounded = torch.cat([matched_reference(cal, x[i:i + 8], False) for i in chunks])
    torch.cuda.synchronize()
    # the same formula twice: equal up to the convolution library's choice of algorithm per call (fp32 summation order)
    drift = float((mine[:, :4] - matched[:, :4]).abs().max())
    assert drift < 0.03 and float((mine[:, 4:] - matched[:, 4:]).abs().max()) < 2e-3, \
        f"this tool's rounding-matched reference drifted from tests/helpers.py ({drift} px)"
    assert torch.equal(h16, h32), "the split plan's head tensor differs from the default plan's"
    assert torch.equal(b32.half().view(torch.int16), h32[:, :4].contiguous().view(torch.int16))
    flips = lambda got: int(((got[:, 4:].float() >= 0.25) != (want[:, 4:] >= 0.25)).sum())       # noqa: E731
    rows16 = h32[:, :4].float()
    rep = {
        "anchors": int(batch * b32.shape[2]), "scores_at_or_above_0.25_in_fp32_module": int((want[:, 4:] >= 0.25).sum()),
        "kernel_selection": "measured" if p16.tuning_source == "measured" else "persisted selection of an earlier run",
        "box_px": {
            "boxes32_vs_fp32_module": _stats(b32 - want[:, :4]), "fp16_rows_vs_fp32_module": _stats(rows16 - want[:, :4]),
            "boxes32_vs_rounding_matched_reference": _stats(b32 - matched[:, :4]),
            "fp16_rows_vs_rounding_matched_reference": _stats(rows16 - matched[:, :4])},
        "box_logit_rounding": {
            "what": "rounding-matched reference in torch against the fp32 module, with and without the fp16 rounding of the box logits",
            "with_rounded_logits_vs_fp32_module": _stats(mine[:, :4] - want[:, :4]),
            "with_unrounded_logits_vs_fp32_module": _stats(unrounded[:, :4] - want[:, :4]),
            "rounded_vs_unrounded_logits": _stats(mine[:, :4] - unrounded[:, :4])},
        "threshold_flips_at_0.25": {"default_mode": flips(h16), "box_rows_fp32": flips(h32), "of_decisions": int(h32[:, 4:].numel())},
    }
    assert rep["threshold_flips_at_0.25"]["default_mode"] == rep["threshold_flips_at_0.25"]["box_rows_fp32"]
    return rep


# ------------------------------------------------------------------------------------------------ pipeline legs (child)
def _runner(depth, box_rows):
    import torch

    from realtime_video_analytics_32streams_amd import ops
    from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
    from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
    from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
    from realtime_video_analytics_32streams_amd.tracker import IouTracker
    from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density
    torch.cuda.set_device(0)
    S = 32
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    det = HipYoloDetector(DetectorConfig(model_path="yolov8s.pt", backend="hip", half=True, warmup=False, confidence_threshold=0.25,
                                         hip_box_rows=box_rows), net=build_detector_net("s", seed=0))
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs[:8]], (640, 640), half=True)
        calibrate_detection_density(det.net, sample.contiguous(memory_format=torch.channels_last), 0.25, 120)
    det.invalidate_engine()
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=S, capacity=1024)
    return PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth, use_graph=True), det


def leg_pipeline(depth, box_rows, seconds):
    import numpy as np
    import torch
    runner, det = _runner(depth, box_rows)
    for _ in range(16):
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    assert det.box_rows == box_rows and runner._captured
    sub, lat = {}, []
    done = k = 0
    t0 = time.perf_counter()
    while True:
        if k - done == runner.depth:
            runner.collect(); lat.append(time.perf_counter() - sub.pop(done)); done += 1
        sub[k] = time.perf_counter()
        runner.submit(); k += 1
        if time.perf_counter() - t0 > seconds and k >= 30:
            break
    while done < k:
        runner.collect(); lat.append(time.perf_counter() - sub.pop(done)); done += 1
    dt = time.perf_counter() - t0
    lat_ms = np.array(lat) * 1e3
    return {"frames_per_s": round(32 * k / dt, 1), "ticks": k, "window_s": round(dt, 2),
            "p50_tick_latency_ms": round(float(np.percentile(lat_ms, 50)), 3), "p99_tick_latency_ms": round(float(np.percentile(lat_ms, 99)), 3)}


def leg_profile(box_rows, ticks):
    """What runs under rocprofv3: depth-1 ticks of the 32 x 1080p configuration (one tick at a time, so kernel times are not
    stretched by other ticks' kernels)."""
    import torch
    runner, _ = _runner(1, box_rows)
    for _ in range(ticks):
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    return {"ticks": ticks}


def kernel_times(stats_dir, ticks):
    """K2 and head-launch rows of a rocprofv3 kernel_stats.csv: calls and per-launch average, and their sums per tick."""
    f = sorted(glob.glob(f"{stats_dir}/**/*kernel_stats.csv", recursive=True))[0]
    out = {}
    for r in csv.DictReader(open(f)):
        name = r["Name"]
        key = None
        if "k2_decode" in name:
            key = "k2_decode_split" if "k2_decode_split" in name else "k2_decode"
        elif "k_conv_gbig<" in name:
            targs = [a.strip() for a in name.split("k_conv_gbig<")[1].split(">")[0].split(",")]
            if len(targs) >= 9 and targs[8] in ("true", "1", "(bool)1"):                       # HEAD = true: box and class branch launches
                key = "fused_head k_conv_gbig<" + ", ".join(targs) + ">"
        elif "k_head" in name:
            key = name.split("(")[0].split("::")[-1]
        if key:
            out[key] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)}
    per_tick = lambda pick: round(sum(v["total_ms"] for k, v in out.items() if pick(k)) * 1e3 / ticks, 2)       # noqa: E731
    return {"ticks": ticks, "k2_us_per_tick": per_tick(lambda k: k.startswith("k2_decode")),
            "head_launches_us_per_tick": per_tick(lambda k: not k.startswith("k2_decode")), "kernels": out}


# ------------------------------------------------------------------------------------------------ driver
_ENV = None


def run_leg(name, limit_s, extra, log, profile_dir=None):
    """One GPU step as a child process under its own time limit; returns the JSON the leg printed last."""
    res = Path(tempfile.mkstemp(prefix="box_rows_leg_", suffix=".json")[1])
    cmd = [sys.executable, str(Path(__file__).resolve()), "--leg", name, "--leg-out", str(res), *extra]
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(profile_dir), "--", *cmd]
    cmd = ["timeout", "-k", "10", str(limit_s), *cmd]
    print("+", " ".join(cmd), flush=True)
    global _ENV
    if _ENV is None:
        _ENV = dict(os.environ, RVA_TUNE_CACHE_DIR=tempfile.mkdtemp(prefix="box_rows_tune_"))
    t0 = time.perf_counter()
    rc = subprocess.call(cmd, cwd=str(ROOT), stdout=log, stderr=subprocess.STDOUT, env=_ENV)
    if rc != 0:
        raise SystemExit(f"leg {name} {' '.join(extra)} failed with exit status {rc}: stopping (nothing more is started on the GPU)")
    out = json.loads(res.read_text())
    res.unlink()
    print(f"  {time.perf_counter() - t0:.1f} s:", json.dumps(out)[:300], flush=True)
    return out


def spread(vals):
    return round((max(vals) - min(vals)) / (sum(vals) / len(vals)) * 100, 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="short windows (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "box_rows_f32.json"))
    ap.add_argument("--log", default=None, help="file that receives the legs' output (default: beside --out)")
    ap.add_argument("--skip", default="", help="comma-separated legs to leave out: accuracy, pipeline, profile")
    ap.add_argument("--leg", choices=["accuracy", "pipeline", "profile"], help=argparse.SUPPRESS)
    ap.add_argument("--leg-out", help=argparse.SUPPRESS)
    ap.add_argument("--scale", default="s", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=32, help=argparse.SUPPRESS)
    ap.add_argument("--depth", type=int, default=4, help=argparse.SUPPRESS)
    ap.add_argument("--box-rows", default="fp16", help=argparse.SUPPRESS)
    ap.add_argument("--seconds", type=float, default=3.0, help=argparse.SUPPRESS)
    ap.add_argument("--ticks", type=int, default=60, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        rep = {"accuracy": lambda: leg_accuracy(args.scale, args.batch),
               "pipeline": lambda: leg_pipeline(args.depth, args.box_rows, args.seconds),
               "profile": lambda: leg_profile(args.box_rows, args.ticks)}[args.leg]()
        Path(args.leg_out).write_text(json.dumps(rep))
        return
    skip = {s for s in args.skip.split(",") if s}
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    log = open(args.log or out_path.with_suffix(".log"), "w")
    out = {"what": __doc__.split("\n")[0]}
    if "accuracy" not in skip:
        out["accuracy"] = {}
        for scale, batch in SIZES:
            out["accuracy"][f"{scale}x{batch}"] = run_leg("accuracy", 420, ["--scale", scale, "--batch", str(batch)], log)
        worst = max(v["box_px"]["boxes32_vs_fp32_module"]["max"] for v in out["accuracy"].values())
        out["largest_boxes32_max_vs_fp32_module_px"] = worst
        out["half_ulp_of_the_fp16_rows_between_256_and_512_px"] = 0.125
    if "pipeline" not in skip:
        sec = 1.0 if args.quick else 3.0
        pl = out["pipeline_32x1080p_yolov8s"] = {}
        for depth in (1, 4):
            runs = {"fp16": [], "fp32": []}
            for _ in range(2):                                       # off, on, off, on: alternated on one box
                for mode in ("fp16", "fp32"):
                    runs[mode].append(run_leg("pipeline", 300, ["--depth", str(depth), "--box-rows", mode, "--seconds", str(sec)], log))
            off = [r["frames_per_s"] for r in runs["fp16"]]
            on = [r["frames_per_s"] for r in runs["fp32"]]
            delta = round((sum(on) / len(on) / (sum(off) / len(off)) - 1) * 100, 2)
            pl[f"depth_{depth}"] = {"box_rows_fp16": runs["fp16"], "box_rows_fp32": runs["fp32"], "spread_between_off_runs_pct": spread(off),
                                    "on_against_off_pct": delta,
                                    "on_slower_than_the_spread_of_the_off_runs": bool(-delta > spread(off))}
    if "profile" not in skip:
        out["kernel_times_depth1"] = {}
        ticks = 20 if args.quick else 60
        # a throw-away run first, under the profiler like the two that count (its cache key differs from an unprofiled run's): the
        # kernel selection is in the cache afterwards and the profiled runs contain no tuning launches
        d = Path(tempfile.mkdtemp(prefix="box_rows_prof_warm_"))
        run_leg("profile", 420, ["--box-rows", "fp16", "--ticks", "2"], log, profile_dir=d)
        shutil.rmtree(d, ignore_errors=True)
        for mode in ("fp16", "fp32"):
            d = Path(tempfile.mkdtemp(prefix=f"box_rows_prof_{mode}_"))
            run_leg("profile", 420, ["--box-rows", mode, "--ticks", str(ticks)], log, profile_dir=d)
            out["kernel_times_depth1"][f"box_rows_{mode}"] = kernel_times(d, ticks)
            shutil.rmtree(d, ignore_errors=True)
    out_path.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
