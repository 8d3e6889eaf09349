#!/usr/bin/env python3
"""SHA-256 of the logits, of every stage tap and of the four ``post`` buffers of the clip plans on seeded networks and seeded
inputs: a record that a change to the shared pieces of the plans (csrc/rva_plan_topo.h, csrc/rva_clip_host.h, csrc/rva_lstm_dev.h,
csrc/rva_clip*.hip) moved no bit.  Run it on the build before and on the build after and compare the files; the digests are no
contract across toolchains and no test reads them.

The cases: ``FusedCnnLstm`` at every ``LSTM_SHAPES`` and ``Fused3dCnn`` at every ``C3D_SHAPES`` of tests/clip_stage_refs.py;
``FusedCnnLstmF16`` at ``ODD`` and ``RAGGED`` of tests/clip_f16_refs.py, created under ``RVA_CLIP16_WLDS`` = 1 and 0;
``Fused3dCnnF16`` at ``ODD`` and ``RAGGED`` of tests/clip3d_f16_refs.py.  ``post`` runs on a table of three result rows, the
middle one without a clip, into zeroed buffers.

GPU only: ``python tools/clip_bits.py --out FILE``.  Anywhere: ``python tools/clip_bits.py --compare FILE FILE [FILE ...]``
(exit status 1 if a digest differs)."""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from resnet_bits import compare, sha  # noqa: E402


def digests(plan, clips, names) -> dict:
    import torch

    from realtime_video_analytics_32streams_amd import ops

    n = int(clips.shape[0])
    logits = plan(clips.to(plan.dev))
    out = {"logits": sha(logits), **{name: sha(plan.stage(name, n)) for name in names}}
    table = torch.tensor([[n - 1, 3840, 2160], [-1, 0, 0], [0, 1920, 1080]], dtype=torch.int32, device=plan.dev)
    post = ops.PostBuffers.allocate(3, 8, plan.dev)
    for t in (post.scores, post.cls, post.boxes, post.counts):
        t.zero_()
    plan.post(logits, table, 3, post)
    torch.cuda.synchronize()
    out.update({f"post.{k}": sha(getattr(post, k)) for k in ("scores", "cls", "boxes", "counts")})
    return out


def run() -> dict:
    from tests import clip3d_f16_refs as C16          # as the refs import each other: one copy of every module
    from tests import clip_f16_refs as L16
    from tests import clip_stage_refs as R

    from realtime_video_analytics_32streams_amd import clip_plan as CP

    lstm_stages, c3d_stages = ("pooled", "partial", "feat", "gx", "h1", "h2"), ("act1", "act2", "partial", "feat")
    out = {}
    for s in R.LSTM_SHAPES:
        H, W, T, _, _, _, cap = s
        net, _, clips = R.lstm_case(s)
        out[f"FusedCnnLstm-{R.shape_id(s)}"] = digests(CP.FusedCnnLstm(net, (H, W), T, cap), clips, lstm_stages)
    for s in R.C3D_SHAPES:
        T, H, W, _, _, cap = s
        net, _, frames = R.c3d_case(s)
        out[f"Fused3dCnn-{R.shape_id(s)}"] = digests(CP.Fused3dCnn(net, (H, W), T, cap), frames.permute(0, 2, 1, 3, 4), c3d_stages)
    for name, case in (("odd", L16.ODD), ("ragged", L16.RAGGED)):
        net, clips = L16.seeded(case)
        B, T, _, H, W = case["clips"]
        for wlds in ("1", "0"):
            os.environ["RVA_CLIP16_WLDS"] = wlds                 # read at plan creation
            out[f"FusedCnnLstmF16-{name}-wlds{wlds}"] = digests(CP.FusedCnnLstmF16(net, (H, W), T, B), clips, lstm_stages)
        del os.environ["RVA_CLIP16_WLDS"]
    for name, case in (("odd", C16.ODD), ("ragged", C16.RAGGED)):
        net, clips = C16.seeded(case)
        B, _, T, H, W = case["clips"]
        out[f"Fused3dCnnF16-{name}"] = digests(CP.Fused3dCnnF16(net, (H, W), T, B), clips, c3d_stages)
    return out


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
