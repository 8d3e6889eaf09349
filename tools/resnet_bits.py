#!/usr/bin/env python3
"""SHA-256 of the logits and of every stage tap of the ResNet plans on seeded networks and seeded inputs: a record that a change
to the host side of the plans (csrc/rva_plan_topo.h, csrc/rva_resnet*.hip, resnet_plan.py) moved no bit.  Run it on the build before
and on the build after and compare the files; the digests are no contract across toolchains and no test reads them.

The cases: ``FusedResNet18`` and ``FusedResNet18F16`` at the shapes of tests/resnet_stage_refs.py (a few frames, odd sizes,
capacity above the batch) and at 8 frames of 224 x 224 (where the larger tiles are picked); ``FusedResNetF16`` with the fused and
with the split shortcut at ``SMALL_BASIC`` and ``SMALL_BOTT`` of tests/resnetx_refs.py.

GPU only: ``python tools/resnet_bits.py --out FILE``.  Anywhere: ``python tools/resnet_bits.py --compare FILE FILE [FILE ...]``
(exit status 1 if a digest differs)."""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(plan, frames, names) -> dict:
    n = int(frames.shape[0])
    return {"logits": sha(plan(frames.to(plan.dev))), **{name: sha(plan.stage(name, n)) for name in names}}


def run() -> dict:
    import resnet_stage_refs as R18
    import resnetx_refs as RX

    from realtime_video_analytics_32streams_amd import resnet_plan as RP
    from realtime_video_analytics_32streams_amd import synth
    from realtime_video_analytics_32streams_amd.classify import ResNet18

    out = {}
    cases = [(f"{B}x{H}x{W}-c{classes}-cap{cap}", cap, *R18.case((B, H, W, classes, cap))[::2]) for B, H, W, classes, cap in R18.SHAPES]
    cases.append(("8x224x224-c1000-cap8", 8, synth.seeded_module(lambda: ResNet18(1000), 340), synth.seeded_clip((8, 3, 224, 224), 390)))
    for name, cap, net, frames in cases:
        for cls in (RP.FusedResNet18, RP.FusedResNet18F16):
            out[f"{cls.__name__}-{name}"] = digests(cls(net, tuple(frames.shape[2:]), cap), frames, RP.STAGE_CODES)
    for case in (RX.SMALL_BASIC, RX.SMALL_BOTT):
        _, _, B, H, W, _, _, seed_x = case
        net, frames = RX.make_net(case), synth.seeded_clip((B, 3, H, W), seed_x)
        for split in (False, True):
            plan = RP.FusedResNetF16(net, (H, W), B, split_shortcut=split)
            out[f"FusedResNetF16-{'split' if split else 'fused'}-{RX.case_id(case)}"] = digests(plan, frames, plan.stage_names)
    return out


def compare(files) -> int:
    runs = [json.loads(Path(f).read_text()) for f in files]
    bad = 0
    for case, want in runs[0].items():
        for f, r in zip(files[1:], runs[1:]):
            for k in sorted(set(want) | set(r.get(case, {}))):
                if want.get(k) != r.get(case, {}).get(k):
                    print(f"DIFFERS {case} {k}: {files[0]} vs {f}")
                    bad += 1
    bad += sum(set(r) != set(runs[0]) for r in runs[1:])
    print(f"{len(files)} runs, {len(runs[0])} cases, {sum(len(v) for v in runs[0].values())} digests each, {bad} differences")
    return 1 if bad else 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the digests to this JSON file (default: print them)")
    ap.add_argument("--compare", nargs="+", default=None, help="digest files to compare; nothing is run")
    args = ap.parse_args(argv)
    if args.compare:
        return compare(args.compare)
    text = json.dumps(run(), indent=1, sort_keys=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
