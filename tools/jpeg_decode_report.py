"""K8, the device JPEG decoder, on 1080p frames -> profiles/jpeg_decode.json.

Input: 1920x1080 frames rendered from ``synth.make_nv12`` (K1's colour conversion at full size), encoded once with Pillow at
quality 85, 4:2:0, WITHOUT restart markers (one lane per picture decodes the scan) and once by K7 at quality 85 (one restart
interval per MCU row: 68 lanes per picture).  1 / 8 / 32 pictures per ``JpegBatchDecoder.decode`` call, to NV12 and to BGR: the
wall time of the call (probe, staging, copy, kernels, status) in five alternated runs after two warm-up runs -- medians and
spread (max - min) -- and the device time per step from the events the call records (``rva_jpeg_dec_times``).  The yardstick is
Pillow's decode of the same bytes on the host, one process.  Also: mean and largest difference between (NV12 output -> K1's BGR)
and the exact BGR output, i.e. what the range mapping and the nearest chroma cost.  Clocks are left alone.
Usage: python tools/jpeg_decode_report.py [--out profiles/jpeg_decode.json]"""
import argparse
import io
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from realtime_video_analytics_32streams_amd import ops, synth  # noqa: E402

RUNS, W, H, UNIQUE = 5, 1920, 1080, 8


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
            "spread_ms": round(max(v) - min(v), 3)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pitch = ((W + 255) // 256) * 256
    surfs = [ops.Nv12Surface.from_numpy(*synth.make_nv12(100 + i, W, H, pitch, tick=i), W, H) for i in range(UNIQUE)]
    bgr = ops.resize_nv12_to_bgr(surfs, (W, H))                                  # [UNIQUE, H, W, 3]
    host = bgr.cpu().numpy()
    streams = {"pillow_q85_no_restart": [], "k7_q85_restart_per_mcu_row": []}
    for i in range(UNIQUE):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(host[i][..., ::-1])).save(buf, "JPEG", quality=85, subsampling=2)
        streams["pillow_q85_no_restart"].append(buf.getvalue())
        streams["k7_q85_restart_per_mcu_row"].append(ops.jpeg_encode_bgr(bgr[i], 85))
    rep = {"device": torch.cuda.get_device_name(0), "frame": [W, H],
           "protocol": f"{RUNS} alternated runs (NV12, BGR, Pillow on the host) after two warm-up runs; wall = host time around one "
                       "JpegBatchDecoder.decode call incl. its status wait; steps = device time between the events the call records; clocks "
                       "left alone; Pillow decodes the same bytes in this process, one thread",
           "rows": [], "nv12_vs_exact_bgr": []}
    dec = ops.JpegBatchDecoder(32, (W, H), 1 << 20)
    for kind, uniq in streams.items():
        info = ops.jpeg_probe(uniq[0])
        for n in (1, 8, 32):
            datas = [uniq[i % UNIQUE] for i in range(n)]
            outs = {"nv12": [ops.Nv12Surface(torch.empty((H, pitch), dtype=torch.uint8, device="cuda"),
                                             torch.empty((H // 2, pitch), dtype=torch.uint8, device="cuda"), W, H) for _ in range(n)],
                    "bgr": [torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]}

            def pillow():
                for d in datas:
                    Image.open(io.BytesIO(d)).load()
            t = {"nv12": [], "bgr": [], "pillow": []}
            steps = {"nv12": [], "bgr": []}
            for run in range(RUNS + 2):
                for fmt in ("nv12", "bgr"):
                    res, ms = wall(lambda: dec.decode(datas, fmt, out=outs[fmt]))
                    assert all(r is not None for r in res), (kind, n, fmt, dec.errors)
                    if run >= 2:
                        t[fmt].append(ms)
                        steps[fmt].append(dec.times())
                t0 = time.perf_counter()
                pillow()
                if run >= 2:
                    t["pillow"].append((time.perf_counter() - t0) * 1e3)
            row = {"streams": kind, "bytes_per_image": int(statistics.mean(len(d) for d in datas)), "lanes_per_image": info["intervals"],
                   "images_per_call": n, "pillow_host": stats(t["pillow"])}
            for fmt in ("nv12", "bgr"):
                row[fmt] = {"wall": stats(t[fmt]),
                            "steps_median_ms": {k: round(statistics.median(s[k] for s in steps[fmt]), 3) for k in steps[fmt][0]},
                            "steps_spread_ms": {k: round(max(s[k] for s in steps[fmt]) - min(s[k] for s in steps[fmt]), 3) for k in steps[fmt][0]}}
            row["fits_33ms_tick"] = {fmt: row[fmt]["wall"]["median_ms"] <= 33.0 for fmt in ("nv12", "bgr")}
            print(json.dumps(row), flush=True)
            rep["rows"].append(row)
            if n == 8:                                                           # the cost of NV12: range mapping and nearest chroma
                via = ops.resize_nv12_to_bgr(outs["nv12"], (W, H)).to(torch.int16)
                diff = (via - torch.stack(outs["bgr"]).to(torch.int16)).abs()
                cost = {"streams": kind, "images": n, "mean_abs_diff": round(float(diff.float().mean()), 4), "max_abs_diff": int(diff.max()),
                        "share_of_values_off_by_more_than_2": round(float((diff > 2).float().mean()), 5)}
                print(json.dumps(cost), flush=True)
                rep["nv12_vs_exact_bgr"].append(cost)
            if args.out:
                Path(args.out).write_text(json.dumps(rep, indent=1) + "\n")
    dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
