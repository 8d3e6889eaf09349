"""Measurement report of the fp16 ResNet-18 plan (``model_type: resnet, half: true, hip_engine: plan / native, hip_resnet_fp16:
true``; engine ``resnet-f16``) -> profiles/resnet_f16_plan.json.

  * the network alone at 224 x 224, 1 / 8 / 32 frames: ``resnet-f16``, ``resnet-f32`` (the same frames in fp32), PyTorch-ROCm fp32
    (what ``hip_engine: auto`` gives this head) and the same module as PyTorch fp16, alternated in one process (device events,
    warm-up, five runs each: the median, all five and their spread), and whether the fp16 plan is faster than the fp32 plan by
    more than the two spreads together;
  * the per-layer split of the fp16 plan from a ``rocprofv3 --kernel-trace --output-format csv`` run of ``--stages-only N``
    (tracing only; pass ``--trace-dir N:DIR``): median us per launch, TF per layer from ``resnet_plan.resnet_flops``, beside the
    fp32 plan's split of profiles/resnet_plan.json where that file has one for the same N;
  * the pipeline: 32 x 1920x1080 NV12 streams through ``PipelinedTicks`` at depth 1 and 4 on the three engines a configuration
    can select (five alternated runs each: frames/s, p50 / p99 tick latency);
  * accuracy: 8 frames (seed 77) against the float64 quantised network (fp16 frames and weights, exact activations) and the
    original float64 module, top-5 flips, the same for PyTorch fp16; and the four end-to-end cases of tests/resnet_f16_refs.py
    against their tolerances.

GPU only: ``python tools/resnet_f16_report.py [--out FILE] [--trace-dir N:DIR ...] [--legs network,accuracy,pipeline]`` /
``--stages-only N``.
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
from realtime_video_analytics_32streams_amd.classify import HipResNetDetector, ResNet18  # noqa: E402
from realtime_video_analytics_32streams_amd.config import DetectorConfig, TrackerConfig  # noqa: E402
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline  # noqa: E402
from realtime_video_analytics_32streams_amd.resnet_plan import FusedResNet18, FusedResNet18F16, resnet_flops  # noqa: E402
from realtime_video_analytics_32streams_amd.tracker import IouTracker  # noqa: E402
from tools.resnet_plan_report import device_ms, pipeline_sources  # noqa: E402

PEAK_F16_TF = 2516.6          # dense fp16 matrix peak
HW, CLASSES, LAUNCHES = (224, 224), 1000, 22
TILES = {"2,2,4": "256x64", "1,2,4": "128x64", "1,2,2": "64x64", "1,1,2": "64x32", "1,1,1": "32x32"}     # (MT, NT, WM) -> pixels x channels
ENGINES = ("resnet-f16", "resnet-f32", "torch-fp32", "torch-fp16")


def network_leg(net):
    p16, p32 = FusedResNet18F16(net, HW, 32), FusedResNet18(net, HW, 32)
    t32 = copy.deepcopy(net).eval().float().cuda().to(memory_format=torch.channels_last)
    t16 = copy.deepcopy(t32).half()
    f = resnet_flops(*HW, CLASSES)
    out = []
    for n in (1, 8, 32):
        x32 = torch.randn((n, 3, *HW), device="cuda").half().float()    # the same values for every engine
        x16 = x32.half()
        idx = torch.arange(n, dtype=torch.int32, device="cuda")

        def run_t32():
            with torch.inference_mode():
                t32(x32)

        def run_t16():
            with torch.inference_mode():
                t16(x16)
        fns = {"resnet-f16": lambda: p16.run(x16, idx, n), "resnet-f32": lambda: p32.run(x32, idx, n), "torch-fp32": run_t32,
               "torch-fp16": run_t16}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        reps = max(5, 64 // n)
        ms = {k: [] for k in fns}
        for _ in range(5):                                              # alternated
            for k, fn in fns.items():
                ms[k].append(device_ms(fn, reps))
        flop = n * f["frame"]
        row = {"frames": n, "gflop": flop / 1e9}
        for k, v in ms.items():
            m = float(np.median(v))
            row[k] = {"ms": m, "ms_all": [round(x, 4) for x in v], "spread_ms": max(v) - min(v), "tflops": flop / m / 1e9}
        row["resnet-f16"]["fraction_of_fp16_peak"] = row["resnet-f16"]["tflops"] / PEAK_F16_TF
        for k in ENGINES[1:]:
            row[f"f16_over_{k}"] = row[k]["ms"] / row["resnet-f16"]["ms"]
        row["faster_than_f32_by_more_than_the_combined_spread"] = bool(
            row["resnet-f32"]["ms"] - row["resnet-f16"]["ms"] > row["resnet-f32"]["spread_ms"] + row["resnet-f16"]["spread_ms"])
        row["beats_torch_fp32_and_fp16"] = bool(row["resnet-f16"]["ms"] < min(row["torch-fp32"]["ms"], row["torch-fp16"]["ms"]))
        out.append(row)
        print(json.dumps(row), flush=True)
    return {"workspace_mb_32_frames": {"resnet-f16": p16.workspace_bytes / 2 ** 20, "resnet-f32": p32.workspace_bytes / 2 ** 20}, "passes": out}


def stages_only(n: int, passes: int = 12):
    plan = FusedResNet18F16(synth.seeded_module(lambda: ResNet18(CLASSES), 1), HW, n)
    x = torch.randn((n, 3, *HW), device="cuda").half()
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    for _ in range(passes):
        plan.run(x, idx, n)
    torch.cuda.synchronize()


def fp32_split(n: int):
    """layer -> us of the fp32 plan's recorded split for ``n`` frames (profiles/resnet_plan.json), or {}."""
    path = ROOT / "profiles" / "resnet_plan.json"
    if not path.exists():
        return {}
    for rec in json.loads(path.read_text()).get("layers") or []:
        if rec and rec.get("frames") == n:
            return {r["layer"]: r["us"] for r in rec["layers"]}
    return {}


def layer_split(trace_dir, n: int):
    """Per-layer median us of the passes in a kernel trace of ``--stages-only n``."""
    files = sorted(Path(trace_dir).rglob("*kernel_trace.csv"))
    if not files:
        return None
    rows = []
    with open(files[0]) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            if re.search(r"k_clip16_stem|k_res16_conv|k_res_mean|k_clip_head", name):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    if not rows or len(rows) % LAUNCHES:
        return {"error": f"{len(rows)} dispatches, not a multiple of {LAUNCHES}"}
    f = resnet_flops(*HW, CLASSES)
    names = ["stem"] + [c[0] for c in f["convs"]] + ["mean", "head"]
    flops = [f["stem"]] + [c[1] for c in f["convs"]] + [0.0, f["head"]]
    passes = [rows[i:i + LAUNCHES] for i in range(0, len(rows), LAUNCHES)][2:]          # the first two warm the caches
    was = fp32_split(n)
    out = []
    for j, (nm, fl) in enumerate(zip(names, flops)):
        us = float(np.median([(p[j][1] - p[j][0]) / 1e3 for p in passes]))
        row = {"layer": nm, "us": us, "gflop": n * fl / 1e9, "tflops": n * fl / us / 1e6, "fraction_of_fp16_peak": n * fl / us / 1e6 / PEAK_F16_TF}
        t = re.search(r"k_res16_conv<(\d), (\d), (\d), (\d), (\d+)>|k_res16_convILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d+)E", passes[0][j][2])
        if t:
            g = [v for v in t.groups() if v is not None]
            row["tile"], row["step_channels"] = TILES[",".join(g[:3])], int(g[4])
        if nm in was:
            row["resnet-f32_us"] = was[nm]
        out.append(row)
    span = float(np.median([(p[-1][1] - p[0][0]) / 1e3 for p in passes]))
    pairs = [(f"down{b}", f"mid{b}") for b in (2, 4, 6)]
    us = {r["layer"]: r["us"] for r in out}
    return {"frames": n, "passes": len(passes), "us_sum": sum(r["us"] for r in out), "us_first_start_to_last_end": span, "layers": out,
            "shortcut_convolutions_us": {d: us[d] for d, _ in pairs},
            "note": "a shortcut convolution reads the input its block's conv1 reads; fusing it into that launch would save its launch and "
                    "its read of the input, at most the us listed here per pass"}


def pipeline_leg(engine, half, key, depth, net, streams, srcs, ticks=120, warm=24):
    S = len(streams)
    dcfg = DetectorConfig(model_path="resnet18.onnx", backend="hip", model_type="resnet", confidence_threshold=-1e9,
                          resnet_num_classes=CLASSES, resnet_top_k=5, input_size=list(HW), half=half, warmup=False, hip_engine=engine,
                          hip_resnet_fp16=key)
    det = HipResNetDetector(dcfg, net=copy.deepcopy(net))
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=S, capacity=256)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth)
    for _ in range(warm):
        runner.submit(); runner.collect()
    torch.cuda.synchronize()
    lat, t_enq = [], {}
    t0 = time.perf_counter()
    done = 0
    for k in range(ticks):
        if k - done == runner.depth:
            runner.collect(); lat.append(time.perf_counter() - t_enq[done]); done += 1
        t_enq[k] = time.perf_counter()
        runner.submit()
    while done < ticks:
        runner.collect(); lat.append(time.perf_counter() - t_enq[done]); done += 1
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"engine": det.engine, "depth": runner.depth, "streams": S, "ticks": ticks, "frames_per_s": ticks * S / el,
            "p50_tick_ms": float(np.percentile(lat, 50) * 1e3), "p99_tick_ms": float(np.percentile(lat, 99) * 1e3)}


def accuracy_leg(net):
    """8 frames of the default shape (seed 77), float64 references on the CPU; then the tests' four end-to-end cases."""
    from tests import resnet_f16_refs as Q
    x = synth.seeded_clip((8, 3, *HW), 77)
    x16 = x.half()
    quant, orig = Q.network64(Q.pack64(net), x16), Q.module64(net, x)
    with torch.inference_mode():
        plan = FusedResNet18F16(net, HW, 8)(x.cuda()).cpu().numpy()
        tor = copy.deepcopy(net).cuda().eval().half().to(memory_format=torch.channels_last)(x16.cuda()).float().cpu().numpy()
    top = lambda v: tuple(np.argsort(v, kind="stable")[-5:][::-1])  # noqa: E731
    res = {"frames": 8, "seed": 77, "smallest_top6_gap": min(Q.top_gaps(quant))}
    for name, v in (("resnet-f16", plan), ("torch-fp16", tor)):
        res[name] = {"max_abs_err_vs_quantised": float(np.abs(v - quant).max()), "max_abs_err_vs_original": float(np.abs(v - orig).max()),
                     "top5_flips_vs_quantised": int(sum(top(a) != top(b) for a, b in zip(v, quant))),
                     "top5_flips_vs_original": int(sum(top(a) != top(b) for a, b in zip(v, orig)))}
    res["test_cases"] = {"TOL_Q": Q.TOL_Q, "TOL_O": Q.TOL_O}
    for case in Q.E2E_CASES:
        cnet, cx, cq, emu, co = Q.e2e(case)
        B, H, W = case[:3]
        got = FusedResNet18F16(cnet, (H, W), B)(cx.cuda()).cpu().numpy()
        res["test_cases"]["x".join(str(v) for v in case)] = {
            "emulation_vs_quantised": float(np.abs(emu - cq).max()), "plan_vs_quantised": float(np.abs(got - cq).max()),
            "emulation_vs_original": float(np.abs(emu - co).max()), "plan_vs_original": float(np.abs(got - co).max()),
            "top5_flips_vs_quantised": int(sum(top(a) != top(b) for a, b in zip(got, cq))), "top6_gaps": Q.top_gaps(cq)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resnet_f16_plan.json"))
    ap.add_argument("--trace-dir", action="append", default=[], help="N:DIR of a rocprofv3 kernel trace of --stages-only N")
    ap.add_argument("--stages-only", type=int, default=0)
    ap.add_argument("--legs", default="network,accuracy,pipeline")
    a = ap.parse_args()
    if a.stages_only:
        stages_only(a.stages_only)
        return
    legs = a.legs.split(",")
    net = synth.seeded_module(lambda: ResNet18(CLASSES), 1)
    f = resnet_flops(*HW, CLASSES)
    rep = {"device": torch.cuda.get_device_name(0), "peak_fp16_tflops": PEAK_F16_TF, "shape": {"hw": list(HW), "classes": CLASSES},
           "gflop_per_frame": f["frame"] / 1e9}
    if "network" in legs:
        rep["network"] = network_leg(net)
    rep["layers"] = [layer_split(d, int(n)) for n, d in (t.split(":", 1) for t in a.trace_dir)]
    if "accuracy" in legs:
        rep["accuracy"] = accuracy_leg(net)
        print(json.dumps(rep["accuracy"]), flush=True)
    if "pipeline" in legs:
        rep["pipeline"] = []
        streams, srcs = pipeline_sources()
        configs = (("plan", True, True), ("plan", False, False), ("auto", False, False))
        for depth in (1, 4):
            runs = []
            for eng, half, key in configs * 5:                       # alternated, five each
                runs.append(pipeline_leg(eng, half, key, depth, net, streams, srcs))
                print(json.dumps(runs[-1]), flush=True)
            for eng in ("resnet-f16", "resnet-f32", "torch"):
                v = [r["frames_per_s"] for r in runs if r["engine"] == eng]
                rep["pipeline"].append({"engine": eng, "depth": depth, "streams": 32, "frames_per_s": float(np.median(v)),
                                        "frames_per_s_all": [round(x, 1) for x in v], "spread": (max(v) - min(v)) / float(np.median(v)),
                                        "p50_tick_ms": float(np.median([r["p50_tick_ms"] for r in runs if r["engine"] == eng])),
                                        "p99_tick_ms": float(np.median([r["p99_tick_ms"] for r in runs if r["engine"] == eng]))})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rep, indent=1) + "\n")


if __name__ == "__main__":
    main()
