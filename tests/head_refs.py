"""Float64 reference, designed logits and derived rounding bounds for the YOLOv8 detect head, shared by
tests/test_head_refs_host.py (CPU: the bounds see the bugs) and tests/test_gpu_head_f64.py (the three copies of the head:
``head_anchor`` in csrc/rva_yolo_ops.hip, the ``HEAD`` epilogue of the 1x1 convolution in csrc/rva_conv.hip, ``k_head_f32`` in
csrc/rva_conv_f32.hip).

Reference: ``head_ref`` is ``yolov8.DetectHead.forward`` written out in float64: softmax over the 16 bins of each of the 4 sides,
expectation against 0..15, anchor (x + 0.5, y + 0.5) in raster order i = y*w + x, xywh = ((x1y1 + x2y2) / 2, x2y2 - x1y1) * stride,
classes through the sigmoid.  The inputs are exactly representable in the kernel's input type, so the reference has no input rounding.

Contract of the kernels: every logit is FINITE.  The fp16 head starts its running maximum at -1e30, not -inf, so an all -inf side
is outside the contract, and so are NaNs; the logit sets below keep to it (they reach +-65504, the largest fp16 numbers).

Logit sets (fixed seed; every (anchor, side) draws on its own, so d[0..3] differ within an anchor):
  uniform    spread 0.2 -- what the seeded plans deliver (spread <= 0.19, largest bin probability 0.07);
  dominant   +12 on one bin t, noise of +-0.25 elsewhere; t cycles through 0..15;
  two_equal  two neighbouring bins t, t+1 at +20, the rest 58..62 below: d = t + 0.5; t cycles through 0..14;
  ties       2..16 bins tied exactly at the maximum, the rest 0.5..6 below;
  offset     a common offset of +-1000 under an integer spread of 0..4 (fp16's spacing there is 0.5 to 1): without the max subtraction
             exp overflows (inf / inf) or underflows (0 / 0);
  spread120  one bin at +60, the rest at -60;
  mixed      every side draws one of the six families.
Class logits: the grid -20 (1/16) 20, -0.0, the smallest fp16 subnormal, +-17, +-88, +-100 and +-65504, shuffled.

Bounds, per element, from a first-order error model in float64 -- never fitted to a kernel's output.  u = 2**-24, x_t = v_t - max,
p_t the float64 softmax, d the expectation:
  * fp16 heads (``__expf``, ``sw / se``): ``__expf(x)`` is the hardware's exp2 (1 ulp) of x * log2e; one rounding of the product plus
    the rounded constant give a relative error <= 2 |x| u, plus 2 u: eps_t = (3 + 2 |x_t|) u.
    tol_d = sum_t p_t |t - d| (eps_t + 20 u) + 32 u   (20 u: 16 additions in each of the two sums plus the division; 32 u: the last
    additions of a value <= 15).
    A box row is a sum or difference of two d and an anchor coordinate < 2**8, times stride:
    tol_box = stride (tol_d[a] + tol_d[b] + 6 * 2**-16)   (three fp32 roundings of values < 256).
    A score: tol_s = (3 + 2 |x|) u s (1 - s) + 4 u s + 2**-126.
  * fp32 head (``expf``, ``v / se`` per bin): the same form with eps_t = 2 u (libm's 1 ulp, doubled) and 40 u for the per-bin
    division and the 16-term weighted sum.
  * outputs stored as fp16 additionally get half an fp16 ulp of |ref| + tol, ulp16(v) = 2**(max(floor(log2 v), -14) - 10); the fp32
    side tensor (``boxes32``) and the fp32 head get tol alone.
  * no element is exempt: no percentile, no mask.

``head_f32_cpu`` restates the kernels in numpy float32, operation by operation (``fast_exp=True``: ``head_anchor``'s order with
``__expf`` modelled as float32 exp2(float32(x * float32(log2e))); ``fast_exp=False``: ``k_head_f32``'s order with a correctly rounded
exp), and carries the mutations the host test applies."""
import json
import os
from pathlib import Path

import numpy as np

U = 2.0 ** -24
BINS = np.arange(16, dtype=np.float64)
LOG2E32 = np.float32(1.4426950408889634)

GEOMETRIES = [(3, 20, 13), (1, 1, 1), (2, 16, 16), (2, 5, 77)]            # (B, h, w): block + tail of 4, h != w; one anchor; one block; wide
GEOMETRY_STRIDE = dict(zip(GEOMETRIES, (16.0, 32.0, 8.0, 32.0)))
HEAD3_CASES = [((20, 13), (10, 7), (5, 4)), ((16, 16), (8, 8), (4, 4))]   # 2 + 1 + 1 blocks with tails; exact blocks
STRIDES = (8.0, 16.0, 32.0)
FAMILIES = ("uniform", "dominant", "two_equal", "ties", "offset", "spread120")
BOX_SETS = FAMILIES + ("mixed",)
PAD_ANCHORS, A0 = 37, 21                                                  # A = h*w + 37, the level at anchor offset 21

MUTANTS = ("bins_interleaved", "swap_bins", "no_max", "anchor_no_half", "mod_h", "swap_d0_d2", "swap_wh_rows", "stride_centre_only",
           "sigmoid_neg", "cls_xor1", "batch0")


def geometry_id(g):
    return "x".join(str(v) for v in g)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def _cycle(n, k, rng):
    """n values of 0..k-1, each as often as the others (to within one), in random order."""
    return rng.permutation(np.arange(n) % k)


def _family(name, n, rng):
    rows = np.arange(n)
    if name == "uniform":
        return rng.uniform(-0.1, 0.1, (n, 16))
    if name == "dominant":
        v = rng.uniform(-0.25, 0.25, (n, 16))
        v[rows, _cycle(n, 16, rng)] += 12.0
        return v
    if name == "two_equal":
        v = -40.0 + rng.integers(-2, 3, (n, 16)).astype(np.float64)
        t = _cycle(n, 15, rng)
        v[rows, t] = 20.0
        v[rows, t + 1] = 20.0
        return v
    if name == "ties":
        m = rng.integers(-3, 4, n).astype(np.float64)
        v = m[:, None] - 0.5 * rng.integers(1, 13, (n, 16))
        k = 2 + _cycle(n, 15, rng)                                        # 2 .. 16 tied bins
        tied = np.argsort(np.argsort(rng.random((n, 16)), 1), 1) < k[:, None]
        return np.where(tied, m[:, None], v)
    if name == "offset":
        base = np.where(_cycle(n, 2, rng) == 0, 1000.0, -1000.0)
        return base[:, None] + rng.integers(0, 5, (n, 16))
    if name == "spread120":
        v = np.full((n, 16), -60.0)
        v[rows, _cycle(n, 16, rng)] = 60.0
        return v
    raise ValueError(name)


def box_logits(name, B, h, w, dtype=np.float16, seed=0):
    """``[B, h, w, 64]`` of ``dtype`` (side s of an anchor = channels 16 s .. 16 s + 15), one of ``BOX_SETS``."""
    rng = np.random.default_rng([seed, BOX_SETS.index(name), B, h, w])
    n = B * h * w * 4
    if name == "mixed":
        pick = _cycle(n, len(FAMILIES), rng)
        v = np.empty((n, 16))
        for k, fam in enumerate(FAMILIES):
            v[pick == k] = _family(fam, n, rng)[pick == k]
    else:
        v = _family(name, n, rng)
    v = v.reshape(B, h, w, 64).astype(dtype)
    assert np.isfinite(v).all()
    return v


def cls_logits(B, h, w, nc, dtype=np.float16, seed=0):
    """``[B, h, w, nc]`` of ``dtype``: the special values first, then the grid, repeated to size and shuffled."""
    rng = np.random.default_rng([seed, 99, B, h, w, nc])
    grid = np.arange(-320, 321) / 16.0
    pool = [np.array([-0.0, 2.0 ** -24, 17.0, -17.0, 88.0, -88.0, 100.0, -100.0, 65504.0, -65504.0]), grid]
    if np.dtype(dtype) == np.float32:
        pool.append(grid[:-1] + 1.0 / 48)                                  # off the fp16 grid
    v = rng.permutation(np.resize(np.concatenate(pool), B * h * w * nc)).reshape(B, h, w, nc).astype(dtype)
    assert np.isfinite(v).all()
    return v


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference and bounds
def _softmax(box):
    box = np.asarray(box, dtype=np.float64)
    B, h, w, c = box.shape
    assert c == 64
    x = box.reshape(B, h * w, 4, 16)
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    p = e / e.sum(-1, keepdims=True)
    return x, p, (p * BINS).sum(-1)                                        # x_t, p_t [B, hw, 4, 16]; d [B, hw, 4]


def _sigmoid(c):
    e = np.exp(-np.abs(c))
    return np.where(c >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _assemble(d, scores, h, w, stride, ax=None, ay=None):
    B, hw = d.shape[:2]
    i = np.arange(hw)
    ax = (i % w + 0.5) if ax is None else ax
    ay = (i // w + 0.5) if ay is None else ay
    x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
    out = np.empty((B, 4 + scores.shape[2], hw), dtype=d.dtype)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = (x1 + x2) / 2 * stride, (y1 + y2) / 2 * stride, (x2 - x1) * stride, (y2 - y1) * stride
    out[:, 4:] = scores.transpose(0, 2, 1)
    return out


def head_ref(box, cls, stride):
    """``box [B, h, w, 64]``, ``cls [B, h, w, nc]`` -> float64 ``[B, 4 + nc, h*w]``."""
    cls = np.asarray(cls, dtype=np.float64)
    B, h, w, nc = cls.shape
    _, _, d = _softmax(box)
    return _assemble(d, _sigmoid(cls.reshape(B, h * w, nc)), h, w, float(stride))


def head_bounds(box, cls, stride, kind):
    """The fp32-only bound ``[B, 4 + nc, h*w]`` of the module docstring; ``kind``: ``"f16"`` (head_anchor and the fused epilogue:
    ``__expf``, ``sw / se``) or ``"f32"`` (k_head_f32: ``expf``, ``v / se`` per bin)."""
    assert kind in ("f16", "f32")
    cls = np.asarray(cls, dtype=np.float64)
    B, h, w, nc = cls.shape
    x, p, d = _softmax(box)
    eps, extra = ((3 + 2 * np.abs(x)) * U, 20 * U) if kind == "f16" else (2 * U, 40 * U)
    tol_d = (p * np.abs(BINS - d[..., None]) * (eps + extra)).sum(-1) + 32 * U
    tx = float(stride) * (tol_d[..., 0] + tol_d[..., 2] + 6 * 2.0 ** -16)
    ty = float(stride) * (tol_d[..., 1] + tol_d[..., 3] + 6 * 2.0 ** -16)
    c = cls.reshape(B, h * w, nc)
    s = _sigmoid(c)
    eps_s = (3 + 2 * np.abs(c)) * U if kind == "f16" else 2 * U
    tol = np.empty((B, 4 + nc, h * w))
    tol[:, 0], tol[:, 1], tol[:, 2], tol[:, 3] = tx, ty, tx, ty
    tol[:, 4:] = (eps_s * s * (1 - s) + 4 * U * s + 2.0 ** -126).transpose(0, 2, 1)
    return tol


def ulp16(v):
    with np.errstate(divide="ignore"):
        return 2.0 ** (np.maximum(np.floor(np.log2(np.abs(v))), -14.0) - 10.0)


def fp16_store_tol(ref, tol):
    """The bound of a value rounded once more, to fp16, when it is stored: tol + half an fp16 ulp of |ref| + tol."""
    return tol + 0.5 * ulp16(np.abs(ref) + tol)


def case(name, geometry, nc, kind, stride):
    """(box logits, class logits, reference, fp32-only bound) of one logit set on one geometry; fp16 inputs for ``kind = "f16"``."""
    B, h, w = geometry
    dtype = np.float16 if kind == "f16" else np.float32
    box, cls = box_logits(name, B, h, w, dtype), cls_logits(B, h, w, nc, dtype)
    return box, cls, head_ref(box, cls, stride), head_bounds(box, cls, stride, kind)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels restated in float32 (and their mutants)
def _exp32(x, fast):
    assert x.dtype == np.float32
    with np.errstate(over="ignore", under="ignore"):
        if fast:
            y = x * LOG2E32
            assert y.dtype == np.float32
            return np.exp2(y.astype(np.float64)).astype(np.float32)
        return np.exp(x.astype(np.float64)).astype(np.float32)


def head_f32_cpu(box, cls, stride, fast_exp=False, mut=None):
    """float32 ``[B, 4 + nc, h*w]``, every operation in float32 in the kernels' order.  ``mut``: one of ``MUTANTS``."""
    assert mut is None or mut in MUTANTS
    f = np.float32
    box, cls = np.asarray(box).astype(f), np.asarray(cls).astype(f)
    B, h, w, nc = cls.shape
    hw = h * w
    if mut == "batch0":                                                   # image b reads the logits of image 0
        box, cls = np.broadcast_to(box[:1], box.shape), np.broadcast_to(cls[:1], cls.shape)
    v = box.reshape(B, hw, 4, 16)
    if mut == "bins_interleaved":                                         # the second uint4 unpacked as x, x, x, x, y, y, y, y
        v = v[..., [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 9, 11, 13, 15]]
    if mut == "swap_bins":                                                # f.x / f.y of one half2 exchanged
        v = v[..., [0, 1, 2, 3, 4, 5, 7, 6, 8, 9, 10, 11, 12, 13, 14, 15]]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mx = v.max(-1, keepdims=True) if mut != "no_max" else f(0)
        e = _exp32(v - mx, fast_exp)
        se = np.zeros(e.shape[:-1], dtype=f)
        for t in range(16):
            se = se + e[..., t]
        acc = np.zeros_like(se)
        if fast_exp:                                                      # head_anchor: sw += e * t; d = sw / se
            for t in range(16):
                acc = acc + e[..., t] * f(t)
            d = acc / se
        else:                                                             # k_head_f32: e += (v / se) * t
            for t in range(16):
                acc = acc + (e[..., t] / se) * f(t)
            d = acc
        assert d.dtype == f
        if mut == "swap_d0_d2":
            d = d[..., [2, 1, 0, 3]]
        i = np.arange(hw)
        div = h if mut == "mod_h" else w
        half = f(0.0) if mut == "anchor_no_half" else f(0.5)
        ax, ay = (i % div).astype(f) + half, (i // div).astype(f) + half
        x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
        s, sc = f(stride), (f(1.0) if mut == "stride_centre_only" else f(stride))
        rows = [(x1 + x2) * f(0.5) * s, (y1 + y2) * f(0.5) * s, (x2 - x1) * sc, (y2 - y1) * sc]      # * 0.5f == / 2.f, exactly
        if mut == "swap_wh_rows":
            rows[2], rows[3] = rows[3], rows[2]
        c = cls.reshape(B, hw, nc)
        scores = f(1.0) / (f(1.0) + _exp32(c if mut == "sigmoid_neg" else -c, fast_exp))
    if mut == "cls_xor1":
        assert nc % 2 == 0
        scores = scores[..., np.arange(nc) ^ 1]
    out = np.empty((B, 4 + nc, hw), dtype=f)
    for r in range(4):
        assert rows[r].dtype == f
        out[:, r] = rows[r]
    assert scores.dtype == f
    out[:, 4:] = scores.transpose(0, 2, 1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# observed / bound
def ratio(got, ref, tol):
    """max |got - ref| / tol over every element; a non-finite value counts as infinitely far."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    with np.errstate(invalid="ignore"):
        r = np.abs(got - ref) / tol
    return float(np.where(np.isfinite(r), r, np.inf).max())


def check(entry, what, got, ref, tol, bad):
    """Print observed / bound of one comparison (tests/clip_stage_refs.report), note it in ``bad`` if it is over 1, and, where the
    environment variable ``RVA_REPORT_DIR`` names an existing directory, keep the largest ratio per entry point in its ``head_f64.json``
    (the record behind profiles/head_f64.json)."""
    import torch

    from tests import clip_stage_refs as R
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float64))
    r = R.report((entry,), what, torch.from_numpy(got), torch.from_numpy(np.ascontiguousarray(ref)),
                 torch.from_numpy(np.ascontiguousarray(tol)), out=bad)
    out = os.environ.get("RVA_REPORT_DIR")
    if out and Path(out).is_dir():
        path = Path(out) / "head_f64.json"
        data = json.loads(path.read_text()) if path.exists() else {}
        rec = data.setdefault(entry, {"comparisons": 0, "max_observed_over_bound": 0.0, "at": ""})
        rec["comparisons"] += 1
        if not r <= rec["max_observed_over_bound"]:
            rec["max_observed_over_bound"], rec["at"] = r, what
        path.write_text(json.dumps(data, indent=1, sort_keys=True))
    return r


def check_rows(entry, what, got, ref, tol, bad):
    """``check`` on the box rows and on the score rows apart (a score's ratio says nothing about a box row's); the larger of the two."""
    got = np.asarray(got)
    return max(check(entry + " box", what, got[:, :4], ref[:, :4], tol[:, :4], bad),
               check(entry + " scores", what, got[:, 4:], ref[:, 4:], tol[:, 4:], bad))
