"""Measurement report of the fp32 3D-CNN clip plan (``model_type: 3d_cnn, half: false, hip_engine: native``) ->
profiles/clip3d_plan.json.

  * the network alone: 1, 8 and 32 clips at 112 x 112, T = 16, plan and torch engine alternated in one process (device events,
    warm-up, five runs each: the median and all five): ms per pass, FLOP from the shapes (clip_plan.clip3d_flops), fraction of the
    157.3 TF fp32 matrix peak.  The torch engine is timed on a ready ``[B,3,T,H,W]`` tensor (no gather, no permute);
  * the plan's per-kernel split (conv1 / conv2 / conv3 / mean / head / top-5) from a ``rocprofv3 --kernel-trace --stats --output-format csv`` run of
    ``--stages-only`` (tracing only, no counters in the same run; pass its output directory with ``--stats-dir``);
  * the 3D-CNN stream of tests/golden/sample-temporal-pipeline.yaml (8 x 3840x2160 NV12, L = 16, stride 1, overlap 0.25,
    112 x 112) through PipelinedTicks, ``hip_engine: native`` against ``auto``: frames/s, clips/s, p50 / p99 tick latency (all
    ticks and the ticks where clips fire);
  * accuracy: max |logit error| of both engines against the float64 module at 112 x 112 and on the golden clips of
    tests/golden/temporal_nets.json, and the number of top-5 sets that differ from float64's.

GPU only: ``python tools/clip3d_plan_report.py [--out FILE] [--stats-dir DIR]`` / ``--stages-only``.
"""
from __future__ import annotations

import argparse
import copy
import csv
import json
import re
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from realtime_video_analytics_32streams_amd import synth  # noqa: E402
from realtime_video_analytics_32streams_amd.clip_plan import Fused3dCnn, clip3d_flops  # noqa: E402
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig  # noqa: E402
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline  # noqa: E402
from realtime_video_analytics_32streams_amd.temporal import Cnn3dNet, HipCNN3DDetector  # noqa: E402
from realtime_video_analytics_32streams_amd.tracker import IouTracker  # noqa: E402
from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream  # noqa: E402

PEAK_F32_TF = 157.3
T, HW = 16, (112, 112)
STAGES = {"k_c3d_conv1": "conv1+pool", "k_c3d_conv2": "conv2+pool", "k_c3d_conv3": "conv3+sums", "k_clip_mean": "mean",
          "k_clip_head": "head", "k_clip_post": "top5"}


def device_ms(fn, reps: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def network_leg(net):
    plan = Fused3dCnn(net, HW, T, 32)
    tnet = copy.deepcopy(net).cuda().eval()
    f = clip3d_flops(*HW, T, 400)
    out = []
    for n in (1, 8, 32):
        x = torch.randn((n, T, 3, *HW), device="cuda")              # the ring's layout: planar frames
        xt = x.permute(0, 2, 1, 3, 4).contiguous()                  # the module's layout, made outside the timed region
        idx = torch.arange(n * T, dtype=torch.int32, device="cuda")
        run_plan = lambda: plan.run(x, idx, n)                      # noqa: E731

        def run_torch():
            with torch.inference_mode():
                tnet(xt)
        for fn in (run_plan, run_torch):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        reps = max(3, 48 // n)
        p, t = [], []
        for _ in range(5):                                          # alternated
            p.append(device_ms(run_plan, reps))
            t.append(device_ms(run_torch, reps))
        flop = n * f["clip"]
        row = {"clips": n, "gflop": flop / 1e9}
        for name, v in (("plan", p), ("torch", t)):
            ms = float(np.median(v))
            row[name] = {"ms": ms, "ms_all": [round(x, 4) for x in v], "tflops": flop / ms / 1e9,
                         "fraction_of_peak": flop / ms / 1e9 / PEAK_F32_TF}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def stages_only():
    net = synth.seeded_module(lambda: Cnn3dNet(400), 1)
    plan = Fused3dCnn(net, HW, T, 8)
    x = torch.randn((8, T, 3, *HW), device="cuda")
    idx = torch.arange(8 * T, dtype=torch.int32, device="cuda")
    rows = torch.tensor([[i, 3840, 2160] for i in range(8)], dtype=torch.int32, device="cuda")
    from realtime_video_analytics_32streams_amd import ops
    post = ops.PostBuffers.allocate(8, 8, "cuda")
    for _ in range(20):
        plan.post(plan.run(x, idx, 8), rows, 8, post)
    torch.cuda.synchronize()


def stage_split(stats_dir):
    files = sorted(Path(stats_dir).rglob("*kernel_stats.csv"))
    if not files:
        return None
    split, kernels = {}, {}
    with open(files[0]) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name") or r.get("KernelName") or ""
            key = next((v for k, v in STAGES.items() if k in name), None)
            if key is None:
                continue
            calls, total_ns = int(r["Calls"]), float(r["TotalDurationNs"])
            kernels[re.search(r"k_(?:c3d|clip)_\w+", name).group(0)] = {"calls": calls, "avg_us": total_ns / calls / 1e3}
            split[key] = split.get(key, 0.0) + total_ns / 20 / 1e3            # per 8-clip pass (20 passes)
    return {"clips": 8, "us_per_pass": split, "kernels": kernels}


def pipeline_leg(engine, ticks=160, warm=48, depth=2, S=8):
    W, H = 3840, 2160
    streams = [StreamConfig(name=f"uhd{i:03d}", url=f"synthetic://{W}x{H}", target_fps=30.0, warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, width=W, height=H, n_unique=2) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    dcfg = DetectorConfig(model_path="resnet3d_kinetics.onnx", backend="hip", model_type="3d_cnn", sequence_length=16,
                          sequence_stride=1, temporal_overlap=0.25, confidence_threshold=-1e9, num_action_classes=400,
                          input_size=[112, 112], half=False, warmup=False, hip_engine=engine)
    torch.manual_seed(1)
    det = HipCNN3DDetector(dcfg, net=Cnn3dNet(400).eval())
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=S, capacity=256)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth)
    for _ in range(warm):
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    lat, fire, t_enq = [], [], {}
    clips = 0

    def finish(k):
        nonlocal clips
        r = runner.collect_result()
        dt = time.perf_counter() - t_enq[k]
        lat.append(dt)
        n = sum(1 for v in r.detections_emitted.values() if v)
        clips += n
        if n:
            fire.append(dt)
    t0 = time.perf_counter()
    done = 0
    for k in range(ticks):
        if k - done == runner.depth:
            finish(done); done += 1
        t_enq[k] = time.perf_counter()
        runner.submit()
    while done < ticks:
        finish(done); done += 1
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"engine": det.engine, "depth": depth, "ticks": ticks, "frames_per_s": ticks * S / el, "clips_per_s": clips / el,
            "p99_tick_ms": float(np.percentile(lat, 99) * 1e3), "p50_tick_ms": float(np.percentile(lat, 50) * 1e3),
            "p99_firing_tick_ms": float(np.percentile(fire, 99) * 1e3) if fire else None, "firing_ticks": len(fire)}


def accuracy_leg(net):
    from tests.helpers import temporal_net
    from tests.conftest import load_golden

    def f64(m, x):
        with torch.inference_mode():
            return copy.deepcopy(m).double().eval()(x.double().cpu()).numpy()

    def top(v):
        return tuple(np.argsort(v, kind="stable")[-5:][::-1])

    def compare(m, x):
        ref = f64(m, x)
        plan = Fused3dCnn(m, tuple(x.shape[3:]), x.shape[2], x.shape[0])(x.cuda()).cpu().numpy()
        with torch.inference_mode():
            tor = copy.deepcopy(m).cuda().eval()(x.cuda()).cpu().numpy()
        res = {"clips": int(x.shape[0]), "shape": list(x.shape[1:])}
        for name, v in (("plan", plan), ("torch", tor)):
            res[name] = {"max_abs_err": float(np.abs(v - ref).max()),
                         "top5_differs": int(sum(top(a) != top(b) for a, b in zip(v, ref)))}
        return res
    out = {"112": compare(net, synth.seeded_clip((8, 3, T, *HW), 77))}
    for c in load_golden("temporal_nets.json"):
        if c["kind"] == "3d_cnn":
            m, x = temporal_net(c)
            r = compare(m, x)
            r["max_abs_err_vs_recorded"] = float(np.abs(Fused3dCnn(m, tuple(x.shape[3:]), x.shape[2], x.shape[0])(x.cuda())
                                                        .cpu().numpy() - np.asarray(c["logits"])).max())
            out[f"golden_c{c['ctor']['num_classes']}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip3d_plan.json"))
    ap.add_argument("--stats-dir", default=None)
    ap.add_argument("--stages-only", action="store_true")
    a = ap.parse_args()
    if a.stages_only:
        stages_only()
        return
    net = synth.seeded_module(lambda: Cnn3dNet(400), 1)
    rep = {"device": torch.cuda.get_device_name(0), "peak_fp32_tflops": PEAK_F32_TF, "shape": {"hw": list(HW), "T": T},
           "flop": clip3d_flops(*HW, T, 400)}
    rep["network"] = network_leg(net)
    if a.stats_dir:
        rep["stages"] = stage_split(a.stats_dir)
    rep["accuracy"] = accuracy_leg(net)
    print(json.dumps(rep["accuracy"]), flush=True)
    rep["pipeline"] = []
    for eng in ("native", "auto", "native", "auto"):
        r = pipeline_leg(eng)
        print(json.dumps(r), flush=True)
        rep["pipeline"].append(r)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rep, indent=1) + "\n")


if __name__ == "__main__":
    main()
