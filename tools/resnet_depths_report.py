"""Measurement report of the any-depth fp16 ResNet plan (``classify.ResNet`` on ``resnet_plan.FusedResNetF16``, engine
``resnet-f16``) -> profiles/resnet_depths.json.

  * ``network``: the network alone for ResNet-34 / 50 / 101 at 224 x 224 and 1 / 8 / 32 frames: this plan fused (the default: a
    block's shortcut convolution inside the launch of its closing convolution), this plan split (``split_shortcut=True``), the
    same module as PyTorch fp16 channels-last and as PyTorch fp32 (what ``hip_engine: auto`` gives), alternated in one process
    (device events, warm-up, five runs each: the median, all five and their spread);
  * ``accuracy``: 8 frames (seed 77) against the float64 quantised network and the original float64 module, with top-5 flips, for
    the fused plan, the split plan and PyTorch fp16;
  * ``launches``: the per-launch table of ResNet-50 x 32 from a ``rocprofv3 --kernel-trace --output-format csv`` run of
    ``--stages-only 32`` (tracing only; pass ``--trace-dir DIR`` for the fused plan and ``--trace-dir-split DIR`` for the split
    one): FLOP and bytes from ``resnet_plan.resnet_any_flops``, median us, TF and GB/s per launch;
  * ``workspace``: the workspace of 32 frames for ResNet-34 / 50 / 101 / 152, fused and split;
  * ``pipeline``: 32 x 1920x1080 NV12 streams through ``PipelinedTicks`` at depth 1 and 4 for ResNet-50, on ``resnet-f16`` and on
    ``hip_engine: auto`` (five alternated runs each);
  * ``regression``: the three network-alone figures of tools/resnet_f16_report.py (the ResNet-18 plan) from a checkout of the
    parent commit (``--parent-tree DIR``, built) and from this tree, alternated as separate processes.

GPU only: ``python tools/resnet_depths_report.py [--out FILE] [--legs network,accuracy,workspace,pipeline,regression]
[--trace-dir DIR] [--trace-dir-split DIR] [--parent-tree DIR]`` / ``--stages-only N [--split]``.  A leg that is not run keeps what
the output file already holds for it.
"""
from __future__ import annotations

import argparse
import copy
import csv
import json
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from realtime_video_analytics_32streams_amd import synth  # noqa: E402
from realtime_video_analytics_32streams_amd.classify import RESNET_DEPTHS, HipResNetDetector, build_resnet  # noqa: E402
from realtime_video_analytics_32streams_amd.config import DetectorConfig, TrackerConfig  # noqa: E402
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline  # noqa: E402
from realtime_video_analytics_32streams_amd.resnet_plan import FusedResNetF16, resnet_any_flops  # noqa: E402
from realtime_video_analytics_32streams_amd.tracker import IouTracker  # noqa: E402
from tools.resnet_plan_report import device_ms, pipeline_sources  # noqa: E402

PEAK_F16_TF = 2516.6          # dense fp16 matrix peak
HW, CLASSES = (224, 224), 1000
ENGINES = ("fused", "split", "torch-fp16", "torch-fp32")


def _flops(depth, split=False):
    block, blocks = RESNET_DEPTHS[depth]
    return resnet_any_flops(block == "bottleneck", blocks, *HW, CLASSES, split_shortcut=split)


def network_leg(depth):
    net = build_resnet(depth, seed=1, num_classes=CLASSES)
    fused, split = FusedResNetF16(net, HW, 32), FusedResNetF16(net, HW, 32, split_shortcut=True)
    t32 = copy.deepcopy(net).eval().float().cuda().to(memory_format=torch.channels_last)
    t16 = copy.deepcopy(t32).half()
    f = _flops(depth)
    out = []
    for n in (1, 8, 32):
        x32 = torch.randn((n, 3, *HW), device="cuda").half().float()    # the same values for every engine
        x16 = x32.half()
        x32cl, x16cl = x32.contiguous(memory_format=torch.channels_last), x16.contiguous(memory_format=torch.channels_last)
        idx = torch.arange(n, dtype=torch.int32, device="cuda")

        def run_t32():
            with torch.inference_mode():
                t32(x32cl)

        def run_t16():
            with torch.inference_mode():
                t16(x16cl)
        fns = {"fused": lambda: fused.run(x16, idx, n), "split": lambda: split.run(x16, idx, n), "torch-fp16": run_t16, "torch-fp32": run_t32}
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
        row = {"depth": depth, "frames": n, "gflop": flop / 1e9}
        for k, v in ms.items():
            m = float(np.median(v))
            row[k] = {"ms": m, "ms_all": [round(x, 4) for x in v], "spread_ms": max(v) - min(v), "tflops": flop / m / 1e9}
        row["fused"]["fraction_of_fp16_peak"] = row["fused"]["tflops"] / PEAK_F16_TF
        for k in ENGINES[1:]:
            row[f"{k}_over_fused"] = row[k]["ms"] / row["fused"]["ms"]
        row["fused_faster_than_split_by_more_than_the_combined_spread"] = bool(
            row["split"]["ms"] - row["fused"]["ms"] > row["split"]["spread_ms"] + row["fused"]["spread_ms"])
        row["split_faster_than_fused_by_more_than_the_combined_spread"] = bool(
            row["fused"]["ms"] - row["split"]["ms"] > row["split"]["spread_ms"] + row["fused"]["spread_ms"])
        out.append(row)
        print(json.dumps(row), flush=True)
    return {"depth": depth, "launches": {"fused": fused.n_launches, "split": split.n_launches}, "passes": out}


def accuracy_leg(depth):
    """8 frames of the default shape (seed 77) against float64 on the CPU."""
    from tests import resnetx_refs as X
    block, blocks = RESNET_DEPTHS[depth]
    bott = block == "bottleneck"
    net = build_resnet(depth, seed=1, num_classes=CLASSES)
    x = synth.seeded_clip((8, 3, *HW), 77)
    x16 = x.half()
    quant, orig = X.network64(X.pack64(net), x16, False, True, bott, blocks), X.module64(net, x)
    with torch.inference_mode():
        fused = FusedResNetF16(net, HW, 8)(x.cuda()).cpu().numpy()
        split = FusedResNetF16(net, HW, 8, split_shortcut=True)(x.cuda()).cpu().numpy()
        tor = copy.deepcopy(net).cuda().eval().half().to(memory_format=torch.channels_last)(x16.cuda()).float().cpu().numpy()
    top = lambda v: tuple(np.argsort(v, kind="stable")[-5:][::-1])  # noqa: E731
    res = {"depth": depth, "frames": 8, "seed": 77, "smallest_top6_gap": min(X.top_gaps(quant)), "largest_logit": float(np.abs(quant).max())}
    for name, v in (("fused", fused), ("split", split), ("torch-fp16", tor)):
        res[name] = {"max_abs_err_vs_quantised": float(np.abs(v - quant).max()), "max_abs_err_vs_original": float(np.abs(v - orig).max()),
                     "top5_flips_vs_quantised": int(sum(top(a) != top(b) for a, b in zip(v, quant))),
                     "top5_flips_vs_original": int(sum(top(a) != top(b) for a, b in zip(v, orig)))}
    res["quantised_vs_original"] = float(np.abs(quant - orig).max())
    return res


def stages_only(n: int, split: bool, depth: int = 50, passes: int = 12):
    plan = FusedResNetF16(build_resnet(depth, seed=1, num_classes=CLASSES), HW, n, split_shortcut=split)
    x = torch.randn((n, 3, *HW), device="cuda").half()
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    for _ in range(passes):
        plan.run(x, idx, n)
    torch.cuda.synchronize()


def launch_table(trace_dir, n: int, split: bool, depth: int = 50):
    """Per-launch median us of the passes in a kernel trace of ``--stages-only n``, beside the launch's FLOP and bytes."""
    files = sorted(Path(trace_dir).rglob("*kernel_trace.csv"))
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    rows = []
    with open(files[0]) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            if re.search(r"k_clip16_stem|k_res16_conv|k_res_mean|k_clip_head", name):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    f = _flops(depth, split)
    names = ["stem"] + [c[0] for c in f["launches"]] + ["mean", "head"]
    per = len(names)
    if not rows or len(rows) % per:
        return {"error": f"{len(rows)} dispatches, not a multiple of {per}"}
    flops = [f["stem"]] + [c[1] for c in f["launches"]] + [0.0, f["head"]]
    nbytes = [None] + [c[2] for c in f["launches"]] + [None, None]
    passes = [rows[i:i + per] for i in range(0, len(rows), per)][2:]               # the first two warm the caches
    out = []
    for j, (nm, fl, by) in enumerate(zip(names, flops, nbytes)):
        us = float(np.median([(p[j][1] - p[j][0]) / 1e3 for p in passes]))
        row = {"launch": nm, "us": us, "gflop": n * fl / 1e9, "tflops": n * fl / us / 1e6}
        if by is not None:
            row["mbytes"], row["gbytes_per_s"] = n * by / 1e6, n * by / us / 1e3
        t = re.search(r"k_res16_convILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d+)ELb([01])E", passes[0][j][2]) or \
            re.search(r"k_res16_conv<(\d), (\d), (\d), (\d), (\d+), (true|false|[01])>", passes[0][j][2])
        if t:
            g = t.groups()
            row["tile"], row["step_channels"], row["dual"] = f"{32 * int(g[0]) * int(g[2])}x{32 * int(g[1])}", int(g[4]), g[5] in ("1", "true")
        out.append(row)
    span = float(np.median([(p[-1][1] - p[0][0]) / 1e3 for p in passes]))
    return {"depth": depth, "frames": n, "split": split, "passes": len(passes), "us_sum": sum(r["us"] for r in out),
            "us_first_start_to_last_end": span, "launches": out}


def pipeline_leg(engine, depth, net, streams, srcs, ticks=120, warm=24):
    S = len(streams)
    dcfg = DetectorConfig(model_path="resnet50.pt", backend="hip", model_type="resnet", confidence_threshold=-1e9,
                          resnet_num_classes=CLASSES, resnet_top_k=5, input_size=list(HW), half=engine != "auto", warmup=False,
                          hip_engine=engine, hip_resnet_fp16=engine != "auto")
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


def regression_leg(parent_tree: str, rounds: int = 3):
    """tools/resnet_f16_report.py --legs network from the parent's tree and from this one, alternated, each a process of its own."""
    trees = {"parent": Path(parent_tree).resolve(), "this": ROOT}
    ms = {k: {n: [] for n in (1, 8, 32)} for k in trees}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            for k, tree in trees.items():
                out = Path(tmp) / f"{k}{r}.json"
                subprocess.run([sys.executable, str(tree / "tools" / "resnet_f16_report.py"), "--legs", "network", "--out", str(out)],
                               cwd=str(tree), check=True, stdout=subprocess.DEVNULL, timeout=300)
                for row in json.loads(out.read_text())["network"]["passes"]:
                    ms[k][row["frames"]].append(row["resnet-f16"]["ms"])
    res = {"what": "resnet-f16 (ResNet-18 plan) network alone at 224 x 224, ms: median of each process's five-run median", "rounds": rounds,
           "frames": []}
    for n in (1, 8, 32):
        a, b = ms["parent"][n], ms["this"][n]
        row = {"frames": n, "parent_ms": float(np.median(a)), "parent_all": [round(v, 4) for v in a], "this_ms": float(np.median(b)),
               "this_all": [round(v, 4) for v in b]}
        row["difference_ms"] = row["this_ms"] - row["parent_ms"]
        row["inside_the_spread"] = bool(abs(row["difference_ms"]) <= (max(a) - min(a)) + (max(b) - min(b)))
        res["frames"].append(row)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resnet_depths.json"))
    ap.add_argument("--trace-dir", default="")
    ap.add_argument("--trace-dir-split", default="")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--stages-only", type=int, default=0)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--legs", default="network,accuracy,workspace,pipeline")
    a = ap.parse_args()
    if a.stages_only:
        stages_only(a.stages_only, a.split)
        return
    legs = a.legs.split(",")
    out = Path(a.out)
    rep = json.loads(out.read_text()) if out.exists() else {}
    rep.update({"device": torch.cuda.get_device_name(0), "peak_fp16_tflops": PEAK_F16_TF, "shape": {"hw": list(HW), "classes": CLASSES},
                "gflop_per_frame": {str(d): _flops(d)["frame"] / 1e9 for d in (34, 50, 101, 152)}})

    def save():
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rep, indent=1) + "\n")

    if "network" in legs:
        rep["network"] = [network_leg(d) for d in (34, 50, 101)]
        save()
    if "accuracy" in legs:
        rep["accuracy"] = []
        for d in (34, 50, 101):
            rep["accuracy"].append(accuracy_leg(d))
            print(json.dumps(rep["accuracy"][-1]), flush=True)
        save()
    if "workspace" in legs:
        rep["workspace_mb_32_frames"] = {}
        for d in (34, 50, 101, 152):
            net = build_resnet(d, seed=1, num_classes=CLASSES)
            rep["workspace_mb_32_frames"][str(d)] = {
                "fused": FusedResNetF16(net, HW, 32).workspace_bytes / 2 ** 20,
                "split": FusedResNetF16(net, HW, 32, split_shortcut=True).workspace_bytes / 2 ** 20,
                "per_frame_from_the_shapes_mb": _flops(d)["workspace_bytes"] / 2 ** 20}
        print(json.dumps(rep["workspace_mb_32_frames"]), flush=True)
        save()
    if a.trace_dir or a.trace_dir_split:
        rep["launches"] = [launch_table(d, 32, s) for d, s in ((a.trace_dir, False), (a.trace_dir_split, True)) if d]
        save()
    if "pipeline" in legs:
        rep["pipeline"] = []
        streams, srcs = pipeline_sources()
        net = build_resnet(50, seed=1, num_classes=CLASSES)
        for depth in (1, 4):
            runs = []
            for eng in ("plan", "auto") * 5:                            # alternated, five each
                runs.append(pipeline_leg(eng, depth, net, streams, srcs))
                print(json.dumps(runs[-1]), flush=True)
            for eng in ("resnet-f16", "torch"):
                v = [r["frames_per_s"] for r in runs if r["engine"] == eng]
                rep["pipeline"].append({"net": "resnet50", "engine": eng, "depth": depth, "streams": 32, "frames_per_s": float(np.median(v)),
                                        "frames_per_s_all": [round(x, 1) for x in v], "spread": (max(v) - min(v)) / float(np.median(v)),
                                        "p50_tick_ms": float(np.median([r["p50_tick_ms"] for r in runs if r["engine"] == eng])),
                                        "p99_tick_ms": float(np.median([r["p99_tick_ms"] for r in runs if r["engine"] == eng]))})
        save()
    if "regression" in legs:
        if not a.parent_tree:
            raise SystemExit("the regression leg needs --parent-tree DIR (a built checkout of the parent commit)")
        rep["regression"] = regression_leg(a.parent_tree)
        print(json.dumps(rep["regression"]), flush=True)
        save()


if __name__ == "__main__":
    main()
