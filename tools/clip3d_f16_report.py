"""Measurement report of the fp16 3D-CNN clip plan (``model_type: 3d_cnn / slow_fast, half: true, hip_engine: native,
hip_clip_fp16: true``; engine ``clip3d-f16``) -> profiles/clip3d_f16_plan.json.

  * the network alone: 1, 8 and 32 clips at 112 x 112, T = 16 and 1 and 8 clips at the sample YAML's 256 x 256, T = 32; the fp16
    plan, the fp32 plan (``clip3d-f32``, on the same clips in fp32) and PyTorch-ROCm ``net.half()`` (on the same fp16 clips, a ready
    ``[B,3,T,H,W]`` tensor) alternated in one process (device events, warm-up, five runs each: the median and all five);
  * the plan's per-kernel split from a ``rocprofv3 --kernel-trace --stats --output-format csv`` run of ``--stages-only`` (tracing
    only; pass its output directory with ``--stats-dir``);
  * the pipeline leg of tools/clip3d_plan_report.py (8 x 3840x2160 NV12, L = 16, stride 1, overlap 0.25, 112 x 112) with
    ``half: true`` on the fp16 plan, against the fp32 plan (``half: false``) and PyTorch fp16 (``hip_engine: auto``): frames/s,
    p50 / p99 tick latency;
  * accuracy at the default shape (8 clips, seeds 31 / 33): max |logit error| against the float64 quantised network (fp16 clips and
    weights, exact activations) and the original float64 module, top-5 flips, and the same for PyTorch fp16.

GPU only: ``python tools/clip3d_f16_report.py [--out FILE] [--stats-dir DIR] [--legs network,accuracy,pipeline]`` /
``--stages-only``.
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
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from realtime_video_analytics_32streams_amd import synth  # noqa: E402
from realtime_video_analytics_32streams_amd.clip_plan import Fused3dCnn, Fused3dCnnF16, clip3d_flops, pack_cnn3d  # noqa: E402
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig  # noqa: E402
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline  # noqa: E402
from realtime_video_analytics_32streams_amd.temporal import Cnn3dNet, HipCNN3DDetector  # noqa: E402
from realtime_video_analytics_32streams_amd.tracker import IouTracker  # noqa: E402
from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream  # noqa: E402

PEAK_F16_TF = 2516.6          # dense fp16 matrix peak
SHAPES = (((112, 112), 16, (1, 8, 32)), ((256, 256), 32, (1, 8)))
STAGES = {"k_c3d16_conv1": "conv1+pool", "k_c3d16_conv2": "conv2+pool", "k_c3d16_conv3": "conv3+sums", "k_clip_mean": "mean",
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
    out = []
    for hw, T, counts in SHAPES:
        cap = max(counts)
        p16, p32 = Fused3dCnnF16(net, hw, T, cap), Fused3dCnn(net, hw, T, cap)
        tnet = copy.deepcopy(net).cuda().eval().half()
        f = clip3d_flops(*hw, T, 400)
        for n in counts:
            x16 = torch.randn((n, T, 3, *hw), device="cuda").half()     # the ring's layout: planar frames
            x32 = x16.float()
            xt = x16.permute(0, 2, 1, 3, 4).contiguous()                # the module's layout, made outside the timed region
            idx = torch.arange(n * T, dtype=torch.int32, device="cuda")

            def run_torch():
                with torch.inference_mode():
                    tnet(xt)
            fns = {"clip3d-f16": lambda: p16.run(x16, idx, n), "clip3d-f32": lambda: p32.run(x32, idx, n), "torch-fp16": run_torch}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            reps = max(3, (48 if T == 16 else 8) // n)
            ms = {k: [] for k in fns}
            for _ in range(5):                                          # alternated
                for k, fn in fns.items():
                    ms[k].append(device_ms(fn, reps))
            flop = n * f["clip"]
            row = {"hw": list(hw), "T": T, "clips": n, "gflop": flop / 1e9}
            for k, v in ms.items():
                m = float(np.median(v))
                row[k] = {"ms": m, "ms_all": [round(x, 4) for x in v], "spread_ms": max(v) - min(v), "tflops": flop / m / 1e9}
            row["clip3d-f16"]["fraction_of_fp16_peak"] = row["clip3d-f16"]["tflops"] / PEAK_F16_TF
            row["f16_over_f32"] = row["clip3d-f32"]["ms"] / row["clip3d-f16"]["ms"]
            row["f16_over_torch_fp16"] = row["torch-fp16"]["ms"] / row["clip3d-f16"]["ms"]
            row["faster_than_f32_by_more_than_the_spread"] = bool(
                row["clip3d-f32"]["ms"] - row["clip3d-f16"]["ms"] > max(row["clip3d-f32"]["spread_ms"], row["clip3d-f16"]["spread_ms"]))
            out.append(row)
            print(json.dumps(row), flush=True)
        del p16, p32, tnet
        torch.cuda.empty_cache()
    return out


def stages_only():
    net = synth.seeded_module(lambda: Cnn3dNet(400), 1)
    hw, T = (112, 112), 16
    plan = Fused3dCnnF16(net, hw, T, 8)
    x = torch.randn((8, T, 3, *hw), device="cuda").half()
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
            kernels[re.search(r"k_(?:c3d16|clip)_\w+", name).group(0)] = {"calls": calls, "avg_us": total_ns / calls / 1e3}
            split[key] = split.get(key, 0.0) + total_ns / 20 / 1e3            # per 8-clip pass (20 passes)
    return {"clips": 8, "hw": [112, 112], "T": 16, "us_per_pass": split, "kernels": kernels,
            "longest": max(split, key=split.get) if split else None}


def pipeline_leg(engine, half, key, ticks=160, warm=48, depth=2, S=8):
    W, H = 3840, 2160
    streams = [StreamConfig(name=f"uhd{i:03d}", url=f"synthetic://{W}x{H}", target_fps=30.0, warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, width=W, height=H, n_unique=2) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    dcfg = DetectorConfig(model_path="resnet3d_kinetics.onnx", backend="hip", model_type="3d_cnn", sequence_length=16,
                          sequence_stride=1, temporal_overlap=0.25, confidence_threshold=-1e9, num_action_classes=400,
                          input_size=[112, 112], half=half, warmup=False, hip_engine=engine, hip_clip_fp16=key)
    torch.manual_seed(1)
    det = HipCNN3DDetector(dcfg, net=Cnn3dNet(400).eval())
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=S, capacity=256)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth)
    for _ in range(warm):
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    lat, fire, t_enq = [], [], {}

    def finish(k):
        r = runner.collect_result()
        dt = time.perf_counter() - t_enq[k]
        lat.append(dt)
        if any(r.detections_emitted.values()):
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
    return {"engine": det.engine, "half": half, "depth": depth, "ticks": ticks, "frames_per_s": ticks * S / el,
            "p50_tick_ms": float(np.percentile(lat, 50) * 1e3), "p99_tick_ms": float(np.percentile(lat, 99) * 1e3),
            "p99_firing_tick_ms": float(np.percentile(fire, 99) * 1e3) if fire else None, "firing_ticks": len(fire)}


def accuracy_leg():
    """8 clips of the default shape, seeds 31 / 33, float64 references on the CPU."""
    net = synth.seeded_module(lambda: Cnn3dNet(400), 31)
    x = synth.seeded_clip((8, 3, 16, 112, 112), 33)
    x16 = x.half()
    p = {k: torch.from_numpy(v).double() for k, v in pack_cnn3d(net, half=True).items()}
    for k in ("conv2_w", "conv3_w"):
        p[k] = p[k].permute(0, 2, 1).reshape(p[k].shape[0], p[k].shape[2], 3, 3, 3).contiguous()
    with torch.inference_mode():
        a = F.max_pool3d(F.conv3d(x16.double(), p["conv1_w"], p["conv1_b"], padding=1).relu(), (1, 2, 2))
        a = F.max_pool3d(F.conv3d(a, p["conv2_w"], p["conv2_b"], padding=1).relu(), 2)
        a = F.conv3d(a, p["conv3_w"], p["conv3_b"], padding=1).relu().mean((2, 3, 4))
        quant = (a @ p["head_w"].T + p["head_b"]).numpy()
        orig = copy.deepcopy(net).double().eval()(x.double()).numpy()
        plan = Fused3dCnnF16(net, (112, 112), 16, 8)(x.cuda()).cpu().numpy()
        tor = copy.deepcopy(net).cuda().eval().half()(x16.cuda()).float().cpu().numpy()

    def top(v):
        return tuple(np.argsort(v, kind="stable")[-5:][::-1])
    srt = np.sort(quant, axis=1)[:, ::-1]
    res = {"clips": 8, "shape": [3, 16, 112, 112], "seeds": [31, 33], "smallest_top6_gap": float((srt[:, :5] - srt[:, 1:6]).min())}
    for name, v in (("clip3d-f16", plan), ("torch-fp16", tor)):
        res[name] = {"max_abs_err_vs_quantised": float(np.abs(v - quant).max()), "max_abs_err_vs_original": float(np.abs(v - orig).max()),
                     "top5_flips_vs_quantised": int(sum(top(a) != top(b) for a, b in zip(v, quant))),
                     "top5_flips_vs_original": int(sum(top(a) != top(b) for a, b in zip(v, orig)))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip3d_f16_plan.json"))
    ap.add_argument("--stats-dir", default=None)
    ap.add_argument("--stages-only", action="store_true")
    ap.add_argument("--legs", default="network,accuracy,pipeline")
    a = ap.parse_args()
    if a.stages_only:
        stages_only()
        return
    legs = a.legs.split(",")
    rep = {"device": torch.cuda.get_device_name(0), "peak_fp16_tflops": PEAK_F16_TF,
           "flop_per_clip": {f"{hw[0]}x{hw[1]}xT{T}": clip3d_flops(*hw, T, 400)["clip"] for hw, T, _ in SHAPES}}
    if "network" in legs:
        rep["network"] = network_leg(synth.seeded_module(lambda: Cnn3dNet(400), 1))
    if a.stats_dir:
        rep["stages"] = stage_split(a.stats_dir)
        print(json.dumps(rep["stages"]), flush=True)
    if "accuracy" in legs:
        rep["accuracy"] = accuracy_leg()
        print(json.dumps(rep["accuracy"]), flush=True)
    if "pipeline" in legs:
        rep["pipeline"] = []
        for eng, half, key in (("native", True, True), ("native", False, False), ("auto", True, False)) * 2:
            r = pipeline_leg(eng, half, key)
            print(json.dumps(r), flush=True)
            rep["pipeline"].append(r)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rep, indent=1) + "\n")


if __name__ == "__main__":
    main()
