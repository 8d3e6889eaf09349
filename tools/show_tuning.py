import sys; sys.path.insert(0, ".")
import torch
from realtime_video_analytics_32streams_amd.engine import FusedYoloV8
from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
eng = FusedYoloV8(build_detector_net(sys.argv[2] if len(sys.argv) > 2 else "s").half().cuda(), B)
from realtime_video_analytics_32streams_amd import _native as N


def name(v):
    n = N.lib().rva_conv_variant_name(v)
    return n.decode() if n else str(v)


tot = 0
seen = {}
for launch, state, desc in eng._tunable:
    seen[desc] = seen.get(desc, 0) + 1
t = {d: (v, us) for d, v, us in eng.tuning}
import re
gap_tot = 0
rows = []
for d, n in seen.items():
    v, us = t[d]
    tot += us * n
    d0 = d
    d = re.sub(r"^head[12]:", "", d)
    mu = re.match(r"up(\d+)\+(\d+)->(\d+) k1s1 (\d+)x(\d+)", d)
    if mu:      # fused upsample + concat source: the low-res part is read at quarter size
        cl, cs, cout, h, w = map(int, mu.groups())
        cin, k, st, ho, wo = cl + cs, 1, 1, h, w
        by = 2 * (B * (h // 2) * (w // 2) * cl + B * h * w * cs + B * h * w * cout)
    else:
        cin, cout, k, st, h, w = map(int, re.match(r"(\d+)->(\d+) k(\d)s(\d) (\d+)x(\d+)", d).groups())
        ho, wo = ((h - 1) // st + 1, (w - 1) // st + 1) if k == 3 else (h // st, w // st)
        by = 2 * (B * h * w * cin + B * ho * wo * cout)
    fl = 2 * B * ho * wo * cout * cin * k * k
    t_hbm, t_mfma = by / 6.0e6, fl / 2.5e9          # us at 6 TB/s achievable HBM, 2.5 PFLOP/s dense fp16
    roof = max(t_hbm, t_mfma)
    gap = (us - roof) * n
    gap_tot += gap
    rows.append((gap, f"{d:24s} x{n} {name(v):14s} {us:7.1f} us  hbm {t_hbm:6.1f}  mfma {t_mfma:6.1f}  x{us/roof:4.1f} of roof  gap*n {gap:7.1f} us"))
for _, r in sorted(rows, reverse=True):
    print(r)
print("sum of gaps to the per-layer roofline:", round(gap_tot, 1), "us")
print("sum conv us per forward:", round(tot, 1))
x = torch.rand((B, 3, 640, 640), device="cuda").half()
for _ in range(3): eng(x)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
e0.record()
for _ in range(10): eng(x)
e1.record(); torch.cuda.synchronize()
print("forward ms:", e0.elapsed_time(e1) / 10)
