"""The launch lists of the fused YOLOv8 / YOLOv5 / YOLO11 plans, as the library reports them -> tests/golden/plan_steps.json.

For every case below the plan is created with ``autotune=False`` (nothing runs) and the tool records ``anchors``, ``out_rows``,
``n_steps``, ``n_tunable``, ``quiet_step``, ``fused_head_lanes()`` and, for every step, ``step_desc(i)`` and ``step_rows(i)``.  The
cases are the smallest that reach every branch of the graph builders of csrc/rva_plan.hip; tests/test_gpu_plan_steps.py holds every
later build to the committed record, so a change of the builders that moves, drops or reshapes a launch shows as a diff of that file.

``--run`` also runs every case of 64 x 96 or 256 x 64 once on a seeded network and a seeded input, every step at variant 0, and
records the SHA-256 of the output bytes (``sha256``; with ``box_rows="fp32"`` the fp32 box tensor goes into the hash as well), and
for a case with static rows the hash of the primed, windowed run behind it (``sha256_primed``).  The kernels use no atomics: the
hashes of two processes, or of two builds that launch the same list on the same layouts, are equal.

GPU only: ``python tools/plan_steps.py [--run] [--only CASE ...] [--out FILE]`` (default: the golden file, without ``--run``)."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
GOLDEN = ROOT / "tests" / "golden" / "plan_steps.json"
SMALL, TALL = (64, 96), (256, 64)
WINDOW = (96, 160)
# the switches that reach the descriptor's flags or the windows from the environment: a case sets the ones it names, the rest are unset
ENV = ("RVA_PLAN_NO_STATIC_ROWS", "RVA_PAIR32", "RVA_NO_STEM2", "RVA_NO_CIN_PAD", "RVA_TUNE_LAYER_OVERLAP", "RVA_SERIAL_HEADS")
NO_FUSION = {"RVA_NO_STEM2": "1", "RVA_PAIR32": "0", "RVA_NO_CIN_PAD": "1"}      # RVA_PLAN_NO_STEM2 | NO_PAIR32 | NO_CIN_PAD


def _case(family, scale, nc=80, hw=SMALL, rows=None, env=None, **kw):
    return dict(family=family, scale=scale, nc=nc, hw=hw, rows=rows, env=env or {}, kw=kw)


CASES = {
    "v8n": _case("v8", "n"),                                    # two-launch stem, Cin 16 declared 32, head3
    "v8s": _case("v8", "s"),                                    # stem2, pair32, fused head on lanes
    "v8n-nc91": _case("v8", "n", nc=91),                        # class width padded to 96
    "v8m-nc20": _case("v8", "m", nc=20),
    "v8n-fp32": _case("v8", "n", precision="fp32"),             # fp32 stem, pools, upsample and per-level head on lanes
    "v8n-1600x1568": _case("v8", "n", hw=(1600, 1568)),         # 50 x 49 = 2450 > 2400 positions at stride 32: three maxpool5
    "v5n": _case("v5", "n"),
    "v5s": _case("v5", "s"),
    "11n": _case("11", "n"),                                    # both C3k2 forms; C2PSA with 2 heads
    "11s": _case("11", "s"),                                    # ... with 4
    "v8s-rows": _case("v8", "s", hw=TALL, rows=WINDOW),         # windows derived from the slice addresses
    "v5s-rows": _case("v5", "s", hw=TALL, rows=WINDOW),
    "11n-rows": _case("11", "n", hw=TALL, rows=WINDOW),
    "v8s-nofusion": _case("v8", "s", env=NO_FUSION),
    "v8s-box32": _case("v8", "s", box_rows="fp32"),             # the side tensor's offset behind 4 + nc rows ...
    "v5s-box32": _case("v5", "s", box_rows="fp32"),             # ... behind 5 + nc
    "11n-box32": _case("11", "n", box_rows="fp32"),
}


def build_plan(name):
    """The case's plan (batch 1, seeded network, no tuner) under the case's environment."""
    from realtime_video_analytics_32streams_amd import engine
    from realtime_video_analytics_32streams_amd.yolo11 import build_detector_net_11
    from realtime_video_analytics_32streams_amd.yolov5 import build_detector_net_v5
    from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net
    c = CASES[name]
    net_of, plan_of = {"v8": (build_detector_net, engine.FusedYoloV8), "v5": (build_detector_net_v5, engine.FusedYoloV5),
                       "11": (build_detector_net_11, engine.FusedYolo11)}[c["family"]]
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(c["env"])
    try:
        plan = plan_of(net_of(c["scale"], seed=3, nc=c["nc"]), 1, hw=c["hw"], autotune=False, **c["kw"])
        if c["rows"]:
            plan.set_static_rows(*c["rows"])
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return plan


def describe(plan) -> dict:
    return {"anchors": plan.A, "out_rows": plan.HEAD_ROWS_EXTRA + plan.nc, "n_steps": plan.n_launches, "n_tunable": len(plan._tunable),
            "quiet_step": plan.quiet_step, "fused_head_lanes": bool(plan.fused_head_lanes()),
            "steps": [[plan.step_desc(i), *plan.step_rows(i)] for i in range(plan.n_launches)]}


def _sha(plan) -> str:
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256(plan.out.cpu().numpy().tobytes())
    if plan.boxes32 is not None:
        h.update(plan.boxes32.cpu().numpy().tobytes())
    return h.hexdigest()


def run_hashes(name, plan) -> dict:
    """One run of the seeded input (a constant border outside the case's static rows), and the primed run behind it."""
    import torch
    c = CASES[name]
    top, bottom = c["rows"] or (0, c["hw"][0])
    x = torch.full((1, 3, *c["hw"]), 0.447)
    x[:, :, top:bottom] = torch.rand((1, 3, bottom - top, c["hw"][1]), generator=torch.Generator().manual_seed(11))
    x = x.to(plan.dtype).cuda()
    plan(x)
    out = {"sha256": _sha(plan)}
    if c["rows"]:
        assert plan.primed
        plan(x)
        out["sha256_primed"] = _sha(plan)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--run", action="store_true", help="also run the small cases once and record the SHA-256 of their outputs")
    ap.add_argument("--only", nargs="*", default=None, help="case names (default: all)")
    ap.add_argument("--out", default=None, help=f"output file (default: {GOLDEN.relative_to(ROOT)}; required with --run)")
    a = ap.parse_args(argv)
    if a.run and not a.out:
        ap.error("--run writes hashes, which are no part of the golden file: name an --out file")
    import torch
    assert torch.cuda.is_available(), "plan_steps.py needs the GPU (the plans are created on it)"
    rec = {}
    for name in a.only or CASES:
        plan = build_plan(name)
        rec[name] = describe(plan)
        if a.run and CASES[name]["hw"] in (SMALL, TALL):
            rec[name].update(run_hashes(name, plan))
        print(f"{name}: {rec[name]['n_steps']} steps, {rec[name]['n_tunable']} tunable" + (f", sha256 {rec[name]['sha256'][:16]}" if "sha256" in rec[name] else ""),
              flush=True)
        del plan
    out = Path(a.out) if a.out else GOLDEN
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"cases": rec}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
