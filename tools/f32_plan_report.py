"""Measurement report of the hand-written fp32 YOLOv8 plan (``half: false, hip_engine: plan``) -> profiles/f32_plan.json.

  * accuracy: the plan and the MIOpen engine (``torch-fp32``) against the fused module in float64 on the CPU, n / s / m x 2 on
    torch.rand inputs with calibrated class biases (max |d box| px, max |d class prob|, threshold flips at 0.25);
  * the network alone: device-event time per forward pass, TFLOP/s and the fraction of the 157.3 TF fp32 MFMA peak, for
    n x 32, s x 32, m x 4 (plan and MIOpen; windows of >= 2 s after warm-up);
  * per-layer times of the plan (s x 32) from ``_launch_tunable`` with the selected variant;
  * 32 x 1080p NV12, YOLOv8s, ``half: false`` through PipelinedTicks: frames/s and p99 tick latency at depth 1-4 (>= 3 s
    windows), and a 30-fps paced run (p50 / p99 from the due time of each tick), plan versus ``torch-fp32``.

GPU only: ``python tools/f32_plan_report.py [--quick]``.
"""
from __future__ import annotations

import argparse
import copy
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from realtime_video_analytics_32streams_amd import ops  # noqa: E402
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig  # noqa: E402
from realtime_video_analytics_32streams_amd.detector import HipYoloDetector  # noqa: E402
from realtime_video_analytics_32streams_amd.engine import FusedYoloV8  # noqa: E402
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline  # noqa: E402
from realtime_video_analytics_32streams_amd.tracker import IouTracker  # noqa: E402
from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream  # noqa: E402
from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net, calibrate_detection_density  # noqa: E402

PEAK_F32_TF = 157.3


def gflop_per_image(net, hw=(640, 640)) -> float:
    """2 x MACs of every convolution at its output size (the stem's 3 input channels included)."""
    macs = 0
    hooks = []

    def hook(m, inp, out):
        nonlocal macs
        macs += out.numel() // out.shape[0] * m.in_channels // m.groups * m.kernel_size[0] * m.kernel_size[1]
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            hooks.append(m.register_forward_hook(hook))
    with torch.inference_mode():
        copy.deepcopy(net).float().cpu()(torch.zeros((1, 3, *hw)))
    for h in hooks:
        h.remove()
    return 2 * macs / 1e9


def calibrated(scale, seed, sample=None):
    net = build_detector_net(scale, seed=seed).fuse().cuda().float()
    with torch.inference_mode():
        if sample is None:
            sample = torch.rand((4, 3, 640, 640), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
        calibrate_detection_density(net, sample.contiguous(memory_format=torch.channels_last), 0.25, 60)
    return net


def errors(out, ref, thr=0.25):
    out = out.detach().cpu().double()
    return {"max_abs_box_px": float((out[:, :4] - ref[:, :4]).abs().max()),
            "max_abs_class_prob": float((out[:, 4:] - ref[:, 4:]).abs().max()),
            "threshold_flips_at_0.25": int(((out[:, 4:] >= thr) != (ref[:, 4:] >= thr)).sum()),
            "scores_within_1e-2_of_threshold": int(((ref[:, 4:] - thr).abs() < 1e-2).sum())}


def accuracy_leg():
    res = {}
    for scale in ("n", "s", "m"):
        net = calibrated(scale, 7)
        x = torch.rand((2, 3, 640, 640), device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
        plan = FusedYoloV8(net, 2, precision="fp32", autotune=False)
        out = plan(x).clone()
        with torch.inference_mode():
            mi = net.to(memory_format=torch.channels_last)(x.contiguous(memory_format=torch.channels_last)).float()
            ref = copy.deepcopy(net).cpu().double()(x.cpu().double())
        res[f"{scale}x2"] = {"plan_f32": errors(out, ref), "torch_fp32_miopen": errors(mi, ref)}
        print(scale, res[f"{scale}x2"], flush=True)
        del plan
    return res


def time_window(fn, seconds):
    """Device-event time per call over a window of >= `seconds` (after 3 warm calls)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(int(seconds / max(time.perf_counter() - t0, 1e-4)), 5)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def network_leg(seconds):
    res = {}
    for scale, B in (("n", 32), ("s", 32), ("m", 4)):
        net = calibrated(scale, 0)
        gf = gflop_per_image(net) * B
        x = torch.rand((B, 3, 640, 640), device="cuda")
        plan = FusedYoloV8(net, B, precision="fp32", autotune=True, tune_overlap=1)
        ms, n = time_window(lambda: plan(x), seconds)
        xc = x.contiguous(memory_format=torch.channels_last)
        netc = net.to(memory_format=torch.channels_last)
        with torch.inference_mode():
            ms_t, n_t = time_window(lambda: netc(xc), seconds)
        row = {"gflop_per_pass": round(gf, 1),
               "plan_f32": {"ms": round(ms, 3), "passes": n, "tflops": round(gf / ms, 2), "fraction_of_fp32_peak": round(gf / ms / PEAK_F32_TF, 3)},
               "torch_fp32_miopen": {"ms": round(ms_t, 3), "passes": n_t, "tflops": round(gf / ms_t, 2),
                                     "fraction_of_fp32_peak": round(gf / ms_t / PEAK_F32_TF, 3)}}
        if scale == "s":
            layers = []
            stream = torch.cuda.current_stream()
            import ctypes as C
            sp = C.c_void_p(stream.cuda_stream)
            for launch, st, desc in plan._tunable:
                v = st["variant"]
                us, _ = time_window(lambda: launch(sp, v), 0.05)
                layers.append([desc, v, round(us * 1e3, 1)])
            row["per_layer_us_plan_f32"] = layers
            row["per_layer_sum_ms"] = round(sum(t for _, _, t in layers) / 1e3, 3)
        res[f"{scale}x{B}"] = row
        print(scale, {k: v for k, v in row.items() if k != "per_layer_us_plan_f32"}, flush=True)
        del plan
    return res


def _pipeline(engine, depth, srcs, streams, net):
    det = HipYoloDetector(DetectorConfig(model_path="yolov8s.pt", backend="hip", half=False, warmup=False, confidence_threshold=0.25,
                                         hip_engine="plan" if engine == "plan" else "auto"), net=copy.deepcopy(net).cpu())
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=len(streams), capacity=1024)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth, use_graph=True,
                            net_graph=engine == "plan")
    return det, runner


def saturated(runner, seconds):
    for _ in range(12):
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    sub, lat = {}, []
    done, k = 0, 0
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
    S = len(runner.pipe.streams)
    lat_ms = np.array(lat) * 1e3
    return {"frames_per_s": round(S * k / dt, 1), "ticks": k, "window_s": round(dt, 2),
            "p50_tick_latency_ms": round(float(np.percentile(lat_ms, 50)), 3), "p99_tick_latency_ms": round(float(np.percentile(lat_ms, 99)), 3)}


def paced(runner, ticks, period=1.0 / 30.0):
    for _ in range(12):
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    lat = np.empty(ticks)
    t0 = time.perf_counter() + 0.05
    for k in range(ticks):
        due = t0 + k * period
        while True:
            now = time.perf_counter()
            if now >= due:
                break
            if due - now > 1.5e-3:
                time.sleep(due - now - 1e-3)
        runner.submit()
        runner.collect()
        lat[k] = time.perf_counter() - due
    lat_ms = lat * 1e3
    return {"ticks": ticks, "p50_ms": round(float(np.percentile(lat_ms, 50)), 3), "p99_ms": round(float(np.percentile(lat_ms, 99)), 3),
            "max_ms": round(float(lat_ms.max()), 3)}


def pipeline_leg(seconds, paced_ticks, depths):
    S = 32
    streams = [StreamConfig(name=f"cam{i:03d}", url="synthetic://1920x1080", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs[:8]], (640, 640), half=False)
    net = calibrated("s", 0, sample)
    res = {}
    for engine in ("plan", "torch-fp32"):
        res[engine] = {}
        for depth in depths:
            det, runner = _pipeline(engine, depth, srcs, streams, net)
            assert det.engine == ("fused-f32" if engine == "plan" else "torch-fp32")
            r = saturated(runner, seconds)
            r["net_streams"] = runner.net_streams
            res[engine][f"depth_{depth}"] = r
            print(engine, depth, r, flush=True)
            del runner, det
            torch.cuda.synchronize()
        det, runner = _pipeline(engine, 1, srcs, streams, net)
        res[engine]["paced_30fps"] = paced(runner, paced_ticks)
        print(engine, "paced", res[engine]["paced_30fps"], flush=True)
        del runner, det
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="short windows (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "f32_plan.json"))
    ap.add_argument("--skip-accuracy", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "GPU only"
    torch.cuda.set_device(0)
    sec = 0.5 if args.quick else 2.0
    out = {"device": torch.cuda.get_device_name(0), "fp32_peak_tflops": PEAK_F32_TF,
           "what": __doc__.split("\n")[0]}
    if not args.skip_accuracy:
        out["accuracy_vs_float64_module"] = accuracy_leg()
    out["network_alone"] = network_leg(sec)
    out["pipeline_32x1080p_yolov8s_half_false"] = pipeline_leg(1.0 if args.quick else 3.0, 60 if args.quick else 300,
                                                               (1, 2) if args.quick else (1, 2, 3, 4))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
