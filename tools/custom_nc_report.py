"""Measurement report of the plans for custom class counts -> profiles/custom_nc.json.

The forward pass alone, YOLOv8s x 32 at 640 x 640 (fp16 plan, autotuned, one pass at a time: device events around 50 passes after a
warm-up), on one seeded input, for nc = 1, 3, 20 and 80 -- and, with ``--parent DIR`` (a checkout of the parent commit with its
library built), the same nc = 80 measurement on the parent's code together with the sha256 of the head tensor on both sides.
Five alternated rounds (this tree's nc = 80, the parent's, this tree's with the parent's kernel selection, this tree's small
class counts; the order within a round is turned round every time); nc = 80 runs in a process of its own on both trees.  Every
figure is the median of the five with all five and their spread.

Recorded, not asserted:
  * ``nc80_head_identical_to_parent``: the nc = 80 head tensor has the parent's sha256 (the shared head kernels gained one uniform
    compare per group of eight class rows and nothing else);
  * ``nc80_within_parent_spread``: |median here - median parent| <= the spread of the parent's own five runs;
  * ``nc80_with_parent_selection``: the two libraries tune apart (the tuning cache key holds the library's digest), so this tree's
    nc = 80 plan is also timed with the parent's kernel selection applied: code against code, ``nc80_selection_differs_in`` lists
    the layer shapes the two tuners chose differently;
  * ``small_nc_not_slower_than_nc80``: nc = 1, 3, 20 are not slower than nc = 80 by more than its spread (fewer class rows to write).
``bench.py --dump-outputs`` holds the detections and tracks of a tick, not the head tensor, so the head's sha256 is taken by this
tool's own forward leg on both trees; ``--bench`` adds the sha256 of the ``--dump-outputs`` files of one short bench run per tree
(the nc = 80 pipeline end to end).

The driver touches no GPU itself: every round of a tree is a child process under its own ``timeout -k 10`` that imports the
package from that tree, and the driver stops at the first child that fails.  GPU only:
``python tools/custom_nc_report.py [--parent DIR] [--bench] [--out FILE]``.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NCS = (1, 3, 20, 80)
BATCH, HW, PASSES, WARM = 32, (640, 640), 50, 10


# ------------------------------------------------------------------------------------------------ forward leg (child)
def leg_forward(root: str, ncs, selection=None):
    sys.path.insert(0, root)
    import torch

    from realtime_video_analytics_32streams_amd.engine import FusedYoloV8
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net
    torch.cuda.set_device(0)
    x = torch.rand((BATCH, 3, *HW), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).half()
    out = {}
    plans = {}
    for nc in ncs:
        # nc = 80 is the default of either tree: the parent's build_detector_net is called as it always was
        net = build_detector_net("s", seed=0) if nc == 80 else build_detector_net("s", seed=0, nc=nc)
        assert net.nc == nc
        plans[nc] = FusedYoloV8(net, BATCH, HW)
        if selection:                                                     # another tree's kernel selection for the same layer shapes
            picks = json.loads(Path(selection).read_text())
            assert [d for d, _ in picks] == [d for _, _, d in plans[nc]._tunable], "the selection belongs to other layer shapes"
            for (_, state, _), (_, v) in zip(plans[nc]._tunable, picks):
                state["variant"] = int(v)
    for nc, plan in plans.items():                                        # one after the other: "alternated" is the driver's rounds
        for _ in range(WARM):
            plan(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(PASSES):
            plan(x)
        e1.record()
        torch.cuda.synchronize()
        head = plan(x)
        torch.cuda.synchronize()
        out[str(nc)] = {"ms": e0.elapsed_time(e1) / PASSES, "head_shape": list(head.shape), "launches": plan.n_launches,
                        "head_sha256": hashlib.sha256(head.cpu().numpy().tobytes()).hexdigest(),
                        "finite": bool(torch.isfinite(head).all()),
                        "selection": [[d, int(st["variant"])] for _, st, d in plan._tunable]}
    print("LEG " + json.dumps(out))


# ------------------------------------------------------------------------------------------------ driver
def child(args, env, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, *args], capture_output=True, text=True, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"custom_nc_report: child {args[:4]} ended with status {p.returncode}; stopping")
    return p.stdout


def forward_round(root: Path, ncs, env, selection=None):
    txt = child([str(Path(__file__).resolve()), "--leg", "forward", "--root", str(root), "--ncs", ",".join(str(n) for n in ncs)] +
                (["--selection", str(selection)] if selection else []), env, 420)
    return json.loads(next(line for line in txt.splitlines() if line.startswith("LEG "))[4:])


def summary(vals):
    import numpy as np
    return {"ms": float(np.median(vals)), "ms_all": [round(v, 4) for v in vals], "spread_ms": max(vals) - min(vals)}


def bench_dump_sha(root: Path, env):
    with tempfile.TemporaryDirectory() as d:
        child([str(root / "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "10", "--no-extras", "--no-other-configs", "--no-cpu-baseline",
               "--dump-outputs", d], env, 420)
        h = hashlib.sha256()
        names = sorted(p.name for p in Path(d).glob("*.npy"))
        for n in names:
            h.update(n.encode()); h.update((Path(d) / n).read_bytes())
        return {"files": names, "sha256": h.hexdigest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--root", default=str(ROOT))
    ap.add_argument("--ncs", default=",".join(str(n) for n in NCS))
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, library built")
    ap.add_argument("--bench", action="store_true", help="also one short bench.py --dump-outputs run per tree")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--selection", default=None, help="(leg) JSON [[desc, variant], ...] to run instead of this tree's own selection")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "custom_nc.json"))
    a = ap.parse_args()
    if a.leg == "forward":
        return leg_forward(a.root, [int(v) for v in a.ncs.split(",")], a.selection)
    with tempfile.TemporaryDirectory() as cache:
        env = dict(os.environ, RVA_TUNE_CACHE_DIR=cache)                # the first round of a tree times the variants, the others reuse them
        here, parent, borrowed = [], [], []
        sel = Path(cache) / "parent_selection.json"
        if a.parent:                                                    # (untimed use: tunes the parent and leaves its selection behind)
            sel.write_text(json.dumps(forward_round(Path(a.parent).resolve(), (80,), env)["80"]["selection"]))
        for i in range(a.rounds):                                       # alternated; nc = 80 in a process of its own on both trees
            legs = [lambda: here.append({**forward_round(ROOT, (80,), env), **forward_round(ROOT, NCS[:-1], env)})]
            if a.parent:
                legs += [lambda: parent.append(forward_round(Path(a.parent).resolve(), (80,), env)),
                         lambda: borrowed.append(forward_round(ROOT, (80,), env, sel)["80"])]
            for leg in (legs if i % 2 else legs[::-1]):                 # and the order within a round turned round every time
                leg()
        rep = {"what": f"forward pass alone, YOLOv8s x {BATCH} at {HW[0]} x {HW[1]}, fp16 plan, autotuned, ms per pass over {PASSES} passes; "
                       f"{a.rounds} alternated rounds, one child process per tree and round",
               "device": None, "nc": {}}
        for nc in NCS:
            rows = [r[str(nc)] for r in here]
            assert len({r["head_sha256"] for r in rows}) == 1, f"nc = {nc}: the head tensor changed between rounds"
            rep["nc"][str(nc)] = {**summary([r["ms"] for r in rows]), "head_shape": rows[0]["head_shape"], "launches": rows[0]["launches"],
                                  "head_sha256": rows[0]["head_sha256"], "finite": all(r["finite"] for r in rows),
                                  "selection": rows[0]["selection"]}
        n80 = rep["nc"]["80"]
        rep["small_nc_not_slower_than_nc80"] = {str(nc): bool(rep["nc"][str(nc)]["ms"] <= n80["ms"] + n80["spread_ms"]) for nc in NCS[:-1]}
        if a.parent:
            rows = [r["80"] for r in parent]
            assert len({r["head_sha256"] for r in rows}) == 1, "parent: the head tensor changed between rounds"
            rep["parent_nc80"] = {**summary([r["ms"] for r in rows]), "head_shape": rows[0]["head_shape"], "launches": rows[0]["launches"],
                                  "head_sha256": rows[0]["head_sha256"], "selection": rows[0]["selection"]}
            # the two trees tune apart (the cache key holds the library's digest): the same code with the parent's selection
            rep["nc80_with_parent_selection"] = {**summary([r["ms"] for r in borrowed]), "head_sha256": borrowed[0]["head_sha256"]}
            rep["nc80_selection_differs_in"] = [[d, v, w] for (d, v), (_, w) in zip(rows[0]["selection"], n80["selection"]) if v != w]
            rep["nc80_head_identical_to_parent"] = rows[0]["head_sha256"] == n80["head_sha256"]
            rep["nc80_within_parent_spread"] = bool(abs(n80["ms"] - rep["parent_nc80"]["ms"]) <= rep["parent_nc80"]["spread_ms"])
            rep["nc80_with_parent_selection_within_parent_spread"] = bool(
                abs(rep["nc80_with_parent_selection"]["ms"] - rep["parent_nc80"]["ms"]) <= rep["parent_nc80"]["spread_ms"])
            if a.bench:
                rep["bench_dump_outputs"] = {"parent": bench_dump_sha(Path(a.parent).resolve(), env), "here": bench_dump_sha(ROOT, env)}
                rep["bench_dump_outputs"]["identical"] = rep["bench_dump_outputs"]["parent"]["sha256"] == rep["bench_dump_outputs"]["here"]["sha256"]
        else:
            rep["parent_nc80"] = "not measured (no --parent)"
        name = child(["-c", "import torch; print(torch.cuda.get_device_name(0))"], env, 120).strip().splitlines()[-1]
        rep["device"] = name
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rep, indent=1) + "\n")
    print(json.dumps(rep, indent=1))


if __name__ == "__main__":
    main()
