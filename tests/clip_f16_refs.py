"""Float64 references and derived bounds for the fp16 CNN-LSTM clip plan (csrc/rva_clip_f16.hip, engine ``clip-f16``), shared by
tests/test_clip_f16_host.py (CPU) and the GPU tests.  Built on tests/clip_stage_refs.py: the same per-stage references, each
computed from the tap of the stage before it, on the fp16 frames and the fp16-rounded weights the plan itself holds, with the fp16
storage bound of tests/clip3d_f16_refs.py (``f16_tol``):

  * ``pooled`` (stored fp16): its fp32 value obeys the fp32 stem's bound ``(147 + 2) u32 (conv(|x|, |w|) + |b|)`` pooled with max
    -- a product of two fp16 values is exact in fp32, so only the additions round, and the kernel's padded K slots are 0 x 0 and
    add nothing -- and the one rounding to fp16 adds ``f16_tol``;
  * ``partial``, ``feat``, ``gx``, ``logits`` are fp32 from fp32: exactly the fp32 plan's bounds, on the fp16 ``pooled`` tap and the
    rounded weights;
  * ``h1`` / ``h2``: ``lstm_bound(lstm_e_ref(...))`` with the fp16-rounded LSTM weights as the weights of both torch LSTMs.

End to end: :func:`network64` is the float64 "quantised network" (fp16 clips, fp16-rounded weights, exact activations) and, with
``round_acts=True``, the float64 "emulation" that additionally rounds ``pooled`` to fp16 as the plan stores it.

TOL_Q / TOL_O are 4 x the largest distance, over the four end-to-end cases, of the float64 emulation to the quantised network /
to the original float64 module and the recorded golden logits, rounded up to two digits.  Measured on the CPU
(tests/test_clip_f16_host.py prints them):

    case          |emu - quantised|   |emu - original|   |emu - recorded|   smallest top-(k+1) gap
    golden-h512   2.7e-7              8.5e-6             8.5e-6             6.2e-4
    golden-h48    7.3e-7              1.7e-5             1.7e-5             4.3e-3
    odd           9.4e-7              1.1e-5             -                  9.6e-3
    ragged        2.3e-7              8.7e-6             -                  5.7e-3

so TOL_Q = 4 x 9.355e-7 = 3.8e-6 and TOL_O = 4 x 1.709e-5 = 6.9e-5, both far below the smallest top-(k+1) gap (6.2e-4): "same top-5
as the quantised network" holds with a margin of over 100 x.  The fp32 rounding of the device kernels comes on top of the
emulation's distance; tools/clip_f16_report.py records what an MI355X leaves of the margin in profiles/clip_f16_plan.json.
"""
import copy
import functools

import numpy as np
import torch

from realtime_video_analytics_32streams_amd.clip_plan import pack_cnn_lstm
from tests import clip_stage_refs as R
from tests.clip3d_f16_refs import f16_tol, top  # noqa: F401  (top: re-exported for the tests)

TOL_Q = 3.8e-6                            # |plan - quantised float64 network|
TOL_O = 6.9e-5                            # |plan - original float64 module| and |plan - recorded golden logits|
F16_STAGES = ("pooled",)
STAGES = ("pooled", "partial", "feat", "gx", "h1", "h2")

ODD = dict(classes=10, hidden=48, seeds=(61, 62), clips=(3, 4, 3, 30, 34))            # [B, T, 3, H, W]
RAGGED = dict(classes=10, hidden=48, seeds=(81, 82), clips=(2, 3, 3, 67, 131))


def pack64(net, half=True):
    """``pack_cnn_lstm(net, half)`` as float64 tensors (the module's own layouts)."""
    return {k: R.f64(v) for k, v in pack_cnn_lstm(net, half=half).items()}


def lstm16_case(shape):
    """The seeded case of ``clip_stage_refs.lstm_case`` for the fp16 plan: the module, its fp16-rounded packed weights (float64)
    and the clips ``[n, T, 3, H, W]`` rounded to fp16 (the ring the plan reads)."""
    net, _, clips = R.lstm_case(shape)
    return net, pack64(net), clips.half()


def stored(name, t):
    """``t`` rounded once to the type the plan stores stage ``name`` in."""
    return R.f64(t).half() if name in F16_STAGES else R.f64(t).float()


def pooled_ref(frames16, p, conv1=None):
    """frames ``[F, 3, H, W]`` -> (pooled ``[F, Hp, Wp, 64]``, bound); ``conv1`` = a precomputed ``stem_conv`` pair."""
    y, t = conv1 if conv1 is not None else R.stem_conv(R.f64(frames16), p)
    a, t = R.stem_pool(y, t)
    return a, f16_tol(a, t)


def lstm16_refs(taps, clips16, p, shape):
    """name -> (float64 reference, bound) for pooled, partial, feat, gx, h1, h2, logits; each stage from the tap before it, as
    ``clip_stage_refs.lstm_refs``.  ``taps = None`` chains the references themselves, each rounded once to its storage type."""
    H, W, T, hidden, classes, n, _ = shape
    out = {}
    tap = (lambda k: taps[k]) if taps is not None else (lambda k: stored(k, out[k][0]))
    out["pooled"] = pooled_ref(R.f64(clips16).flatten(0, 1), p)
    y, t = R.conv2_map(tap("pooled"), p)
    out["partial"] = R.partial_from_map(y, t)
    out["feat"] = R.feat_from_partial(tap("partial"), y.shape[2] * y.shape[3])
    out["gx"] = R.gx_from_feat(tap("feat"), p, n, T)
    e_ref = R.lstm_e_ref(tap("feat"), p, n, T)
    h1, h2 = R.lstm(tap("gx"), p)
    b = torch.full_like(h1, R.lstm_bound(e_ref))
    out["h1"], out["h2"] = (h1, b), (h2, b)
    out["logits"] = R.head(R.f64(tap("h2"))[T - 1], p)
    out["_lstm"] = (e_ref, R.lstm_bound(e_ref))
    return out


def network64(p, clips, round_acts=False):
    """Logits ``[B, classes]`` in float64 of packed weights ``p`` on clips ``[B, T, 3, H, W]`` (used as they are): exact
    activations, or with ``round_acts`` ``pooled`` rounded to fp16 as the plan stores it."""
    x = R.f64(clips)
    B, T = x.shape[:2]
    pooled = R.stem_pool(*R.stem_conv(x.flatten(0, 1), p))[0]
    if round_acts:
        pooled = pooled.half().double()
    feat = R.conv2_map(pooled, p)[0].relu().flatten(2).mean(2)
    gx = R.gx_from_feat(feat, p, B, T)[0]
    h2 = R.lstm(gx, p)[1]
    return R.head(h2[T - 1], p)[0].numpy()


def module64(net, clips):
    """The original module in float64 on clips ``[B, T, 3, H, W]``."""
    with torch.inference_mode():
        return copy.deepcopy(net).double().eval()(R.f64(clips)).numpy()


def seeded(case):
    """(net, fp32 clips ``[B, T, 3, H, W]``) of ODD / RAGGED."""
    from realtime_video_analytics_32streams_amd import synth
    from realtime_video_analytics_32streams_amd.temporal import CnnLstmNet
    return (synth.seeded_module(lambda: CnnLstmNet(case["classes"], case["hidden"]), case["seeds"][0]),
            synth.seeded_clip(case["clips"], case["seeds"][1]))


E2E_NAMES = ("golden-h512", "golden-h48", "odd", "ragged")          # the end-to-end cases of tests/test_gpu_clip_f16_plan.py


@functools.lru_cache(maxsize=None)
def e2e(name):
    """(net, fp32 clips, quantised, emulation, original, recorded or None): one end-to-end case and its float64 logits, computed
    once and shared (callers leave them unchanged)."""
    from tests.conftest import load_golden
    from tests.helpers import temporal_net
    if name.startswith("golden"):
        case = {f"golden-h{c['ctor']['hidden_size']}": c for c in load_golden("temporal_nets.json") if c["kind"] == "cnn_lstm"}[name]
        net, x = temporal_net(case)
        x = x.float()
        recorded = np.asarray(case["logits"], np.float64)
    else:
        (net, x), recorded = seeded({"odd": ODD, "ragged": RAGGED}[name]), None
    p, x16 = pack64(net), x.half()
    return net, x, network64(p, x16), network64(p, x16, round_acts=True), module64(net, x), recorded


def top_gap(logits):
    """Smallest gap between consecutive values among the top k + 1 of any row, k = min(5, classes - 1)."""
    gaps = []
    for r in logits:
        s = np.sort(r)[::-1]
        k = min(5, len(r) - 1)
        gaps.append(float(np.min(s[:k] - s[1:k + 1])))
    return min(gaps)
