"""Measurement report of the fp16 CNN-LSTM clip plan (``model_type: cnn_lstm, half: true, hip_engine: plan / native,
hip_lstm_fp16: true``; engine ``clip-f16``) -> profiles/clip_f16_plan.json.

  * the network alone: 1, 8 and 32 clips at 224 x 224, T = 16; the fp16 plan, the fp32 plan (``clip-f32``, on the same clips in
    fp32) and PyTorch-ROCm ``net.half()`` (on the same fp16 clips; what this configuration gets with ``hip_engine: auto``)
    alternated in one process (device events, warm-up, five runs each: the median and all five);
  * the plan's per-kernel split from a ``rocprofv3 --kernel-trace --stats --output-format csv`` run of ``--stages-only`` (tracing
    only; pass its output directory with ``--stats-dir``), beside the fp32 plan's split of profiles/clip_plan.json;
  * the pipeline leg of tools/clip_plan_report.py (BASELINE configs[4]: 8 x 3840x2160 NV12, L = 16, stride 2, overlap 0.5,
    224 x 224) with ``half: true`` on the fp16 plan, against the fp32 plan (``half: false``) and PyTorch fp16 (``hip_engine:
    auto``): frames/s, p50 / p99 tick latency;
  * accuracy at the default shape (8 clips, seeds 31 / 33): max |logit error| against the float64 quantised network (fp16 clips and
    weights, exact activations) and the original float64 module, top-5 flips, and the same for PyTorch fp16; and the four
    end-to-end cases of tests/clip_f16_refs.py against their tolerances.

GPU only: ``python tools/clip_f16_report.py [--out FILE] [--stats-dir DIR] [--legs network,accuracy,pipeline]`` /
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

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from realtime_video_analytics_32streams_amd import synth  # noqa: E402
from realtime_video_analytics_32streams_amd.clip_plan import FusedCnnLstm, FusedCnnLstmF16, clip_flops  # noqa: E402
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig  # noqa: E402
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline  # noqa: E402
from realtime_video_analytics_32streams_amd.temporal import CnnLstmNet, HipCNNLSTMDetector  # noqa: E402
from realtime_video_analytics_32streams_amd.tracker import IouTracker  # noqa: E402
from realtime_video_analytics_32streams_amd.video_stream import SyntheticNv12Stream  # noqa: E402

PEAK_F16_TF = 2516.6          # dense fp16 matrix peak
SHAPES = (((224, 224), 16, (1, 8, 32)),)
STAGES = {"k_clip16_stem": "stem", "k_clip16_conv2": "conv2+sums", "k_clip_mean": "mean", "k_clip16_xproj": "xproj", "k_clip16_lstm": "lstm",
          "k_clip_head": "head", "k_clip_post": "top5"}
F32_SPLIT_US = {"stem": 1059.0, "conv2+mean": 597.0, "lstm": 360.0, "top5": 69.0, "head": 19.0}   # profiles/clip_plan.json, 8 clips


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
        p16, p32 = FusedCnnLstmF16(net, hw, T, cap), FusedCnnLstm(net, hw, T, cap)
        tnet = copy.deepcopy(net).cuda().eval().half()
        f = clip_flops(*hw, T, 512, 400)
        for n in counts:
            x16 = torch.randn((n, T, 3, *hw), device="cuda").half()     # the ring's layout: planar frames
            x32 = x16.float()
            idx = torch.arange(n * T, dtype=torch.int32, device="cuda")

            def run_torch():
                with torch.inference_mode():
                    tnet(x16)
            fns = {"clip-f16": lambda: p16.run(x16, idx, n), "clip-f32": lambda: p32.run(x32, idx, n), "torch-fp16": run_torch}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            reps = max(3, 48 // n)
            ms = {k: [] for k in fns}
            for _ in range(5):                                          # alternated
                for k, fn in fns.items():
                    ms[k].append(device_ms(fn, reps))
            flop = n * f["clip"]
            row = {"hw": list(hw), "T": T, "clips": n, "gflop": flop / 1e9}
            for k, v in ms.items():
                m = float(np.median(v))
                row[k] = {"ms": m, "ms_all": [round(x, 4) for x in v], "spread_ms": max(v) - min(v), "tflops": flop / m / 1e9}
            row["clip-f16"]["fraction_of_fp16_peak"] = row["clip-f16"]["tflops"] / PEAK_F16_TF
            row["f16_over_f32"] = row["clip-f32"]["ms"] / row["clip-f16"]["ms"]
            row["f16_over_torch_fp16"] = row["torch-fp16"]["ms"] / row["clip-f16"]["ms"]
            row["faster_than_f32_by_more_than_the_spread"] = bool(
                row["clip-f32"]["ms"] - row["clip-f16"]["ms"] > max(row["clip-f32"]["spread_ms"], row["clip-f16"]["spread_ms"]))
            out.append(row)
            print(json.dumps(row), flush=True)
        del p16, p32, tnet
        torch.cuda.empty_cache()
    return out


def stages_only():
    net = synth.seeded_module(lambda: CnnLstmNet(400), 1)
    hw, T = (224, 224), 16
    plan = FusedCnnLstmF16(net, hw, T, 8)
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
            kernels[re.search(r"k_clip(?:16)?_\w+", name).group(0)] = {"calls": calls, "avg_us": total_ns / calls / 1e3}
            split[key] = split.get(key, 0.0) + total_ns / 20 / 1e3            # per 8-clip pass (20 passes)
    return {"clips": 8, "hw": [224, 224], "T": 16, "us_per_pass": split, "kernels": kernels,
            "longest": max(split, key=split.get) if split else None, "clip-f32_us_per_pass": F32_SPLIT_US}


def pipeline_leg(engine, half, key, ticks=160, warm=48, depth=2, S=8):
    W, H = 3840, 2160
    streams = [StreamConfig(name=f"uhd{i:03d}", url=f"synthetic://{W}x{H}", target_fps=30.0, warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, width=W, height=H, n_unique=2) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    dcfg = DetectorConfig(model_path="cnn_lstm_kinetics400.onnx", backend="hip", model_type="cnn_lstm", sequence_length=16,
                          sequence_stride=2, temporal_overlap=0.5, confidence_threshold=-1e9, num_action_classes=400,
                          input_size=[224, 224], half=half, warmup=False, hip_engine=engine, hip_lstm_fp16=key)
    torch.manual_seed(1)
    det = HipCNNLSTMDetector(dcfg, net=CnnLstmNet(400).eval())
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
    """8 clips of the default shape, seeds 31 / 33, float64 references on the CPU; then the tests' four end-to-end cases."""
    from tests import clip_f16_refs as Q
    net = synth.seeded_module(lambda: CnnLstmNet(400), 31)
    x = synth.seeded_clip((8, 16, 3, 224, 224), 33)
    x16 = x.half()
    quant, orig = Q.network64(Q.pack64(net), x16), Q.module64(net, x)
    with torch.inference_mode():
        plan = FusedCnnLstmF16(net, (224, 224), 16, 8)(x.cuda()).cpu().numpy()
        tor = copy.deepcopy(net).cuda().eval().half()(x16.cuda()).float().cpu().numpy()

    def top(v):
        return tuple(np.argsort(v, kind="stable")[-5:][::-1])
    res = {"clips": 8, "shape": [16, 3, 224, 224], "seeds": [31, 33], "smallest_top6_gap": Q.top_gap(quant)}
    for name, v in (("clip-f16", plan), ("torch-fp16", tor)):
        res[name] = {"max_abs_err_vs_quantised": float(np.abs(v - quant).max()), "max_abs_err_vs_original": float(np.abs(v - orig).max()),
                     "top5_flips_vs_quantised": int(sum(top(a) != top(b) for a, b in zip(v, quant))),
                     "top5_flips_vs_original": int(sum(top(a) != top(b) for a, b in zip(v, orig)))}
    res["test_cases"] = {"TOL_Q": Q.TOL_Q, "TOL_O": Q.TOL_O}
    for name in Q.E2E_NAMES:
        cnet, cx, cq, emu, co, rec = Q.e2e(name)
        B, T, _, H, W = cx.shape
        got = FusedCnnLstmF16(cnet, (H, W), T, B)(cx.cuda()).cpu().numpy()
        res["test_cases"][name] = {"emulation_vs_quantised": float(np.abs(emu - cq).max()), "plan_vs_quantised": float(np.abs(got - cq).max()),
                                   "emulation_vs_original": float(np.abs(emu - co).max()), "plan_vs_original": float(np.abs(got - co).max()),
                                   "plan_vs_recorded": float(np.abs(got - rec).max()) if rec is not None else None,
                                   "smallest_top6_gap": Q.top_gap(cq)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip_f16_plan.json"))
    ap.add_argument("--stats-dir", default=None)
    ap.add_argument("--stages-only", action="store_true")
    ap.add_argument("--legs", default="network,accuracy,pipeline")
    a = ap.parse_args()
    if a.stages_only:
        stages_only()
        return
    legs = a.legs.split(",")
    rep = {"device": torch.cuda.get_device_name(0), "peak_fp16_tflops": PEAK_F16_TF,
           "flop_per_clip": {f"{hw[0]}x{hw[1]}xT{T}": clip_flops(*hw, T, 512, 400)["clip"] for hw, T, _ in SHAPES},
           "bytes": {k: v for k, v in clip_flops(224, 224, 16, 512, 400, half=True).items() if "bytes" in k}}
    if "network" in legs:
        rep["network"] = network_leg(synth.seeded_module(lambda: CnnLstmNet(400), 1))
    if a.stats_dir:
        rep["stages"] = stage_split(a.stats_dir)
        print(json.dumps(rep["stages"]), flush=True)
    if "accuracy" in legs:
        rep["accuracy"] = accuracy_leg()
        print(json.dumps(rep["accuracy"]), flush=True)
    if "pipeline" in legs:
        rep["pipeline"] = []
        for eng, half, key in (("plan", True, True), ("plan", False, False), ("auto", True, False)) * 2:
            r = pipeline_leg(eng, half, key)
            print(json.dumps(r), flush=True)
            rep["pipeline"].append(r)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rep, indent=1) + "\n")


if __name__ == "__main__":
    main()
