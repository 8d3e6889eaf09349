"""References, fp32 restatements and bounds for the two YOLOv5 kernels (``rva_stem6_conv_f16``, ``rva_conv1x1_head5_f16``),
shared by tests/test_yolov5_host.py (CPU: the bounds reject planted errors) and tests/test_gpu_yolov5_prims.py.

Stem: 6x6 stride 2 pad 2 + bias + SiLU on fp16 planar input.  ``stem6_f64`` is the float64 result from the fp16-rounded inputs
and weights, with ``mag = sum |x w| + |b|`` per output.  Bound per entry (SiLU' <= 1.1; 128 = the padded K; fast-exp SiLU):
    2^-11 |ref| + 1.1 * 128 * 2^-24 * mag + 2^-21 |ref|
Head: ``logits_f64`` is the float64 1x1 convolution, ``head5_decode`` the decode (any float type), ``head5_bound`` pushes the
logit error  dz = Cin * 2^-24 * mag + 2^-11 |z|  (fp32 accumulation of Cin exact products; the epilogue reads the logit staged as
fp16) through the decode's derivative in float64 -- y' = y (1 - y);  xy: 2 stride y';  wh: 8 y y' anchor;  others: y' -- and adds
the output rounding: ulp16(ref) / 2 for the fp16 head, 2^-22 |ref| for ``boxes32``.  Nothing is fitted to a kernel's output.

``stem6_f32_cpu`` / ``head5_f32_cpu`` restate the kernels in numpy float32 with the same rounding points (``__expf`` modelled as
float32 exp2 of float32(x * float32(log2 e))) and take a ``mut=`` hook that plants one error, as ``head_refs.head_f32_cpu`` does."""
import numpy as np

U = 2.0 ** -24
LOG2E32 = np.float32(1.4426950408889634)
DEFAULT_ANCHORS = np.array([[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]], dtype=np.float64).reshape(3, 3, 2)
STRIDES = (8.0, 16.0, 32.0)
STEM_MUTANTS = ("tap_shift", "pad3")
HEAD_MUTANTS = ("swap_xy", "grid_zero", "wrong_level", "no_square")


def check(entry, what, got, ref, tol, bad):
    """max |got - ref| / tol over all elements, printed; a ratio above 1 is appended to ``bad`` (the test asserts ``not bad`` at its
    end, after every comparison has been printed).  Where ``RVA_REPORT_DIR`` names an existing directory the largest ratio per
    ``entry`` is kept in its ``yolov5_bounds.json`` (the record behind profiles/yolov5_plan.json)."""
    import json
    import os
    from pathlib import Path
    got, ref, tol = (np.asarray(v, dtype=np.float64) for v in (got, ref, tol))
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / tol)
    r = float(np.nanmax(ratio)) if np.isfinite(got).all() else float("inf")
    print(f"[{entry}] {what}: max |d| {float(err.max()):.4g}, max observed / bound {r:.3f}")
    if not r <= 1.0:
        bad.append((entry, what, r))
    out = os.environ.get("RVA_REPORT_DIR")
    if out and Path(out).is_dir():
        path = Path(out) / "yolov5_bounds.json"
        data = json.loads(path.read_text()) if path.exists() else {}
        rec = data.setdefault(entry, {"comparisons": 0, "max_observed_over_bound": 0.0, "at": ""})
        rec["comparisons"] += 1
        if not r <= rec["max_observed_over_bound"]:
            rec["max_observed_over_bound"], rec["at"] = r, what
        path.write_text(json.dumps(data, indent=1, sort_keys=True))
    return r


def ulp16(v):
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def _fast_sigmoid32(z):
    z = z.astype(np.float32)
    with np.errstate(over="ignore"):
        e = np.exp2((-z * LOG2E32).astype(np.float32)).astype(np.float32)
        return (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ stem
def _taps(x, Ho, Wo, pad, dtype):
    """``[B, 3, 6, 6, Ho, Wo]``: tap (c, ky, kx) of every output pixel, zero outside the image."""
    B, _, H, W = x.shape
    xp = np.zeros((B, 3, H + 2 * pad + 6, W + 2 * pad + 6), dtype=dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    out = np.empty((B, 3, 6, 6, Ho, Wo), dtype=dtype)
    for ky in range(6):
        for kx in range(6):
            out[:, :, ky, kx] = xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
    return out


def stem6_f64(x16, w16, b32):
    """``x16`` [B,3,H,W] fp16, ``w16`` [Cout,3,6,6] fp16, ``b32`` [Cout] fp32 -> (SiLU output, mag), both [B, H/2, W/2, Cout] float64."""
    B, _, H, W = x16.shape
    t = _taps(x16.astype(np.float64), H // 2, W // 2, 2, np.float64)
    w = w16.astype(np.float64)
    pre = np.einsum("bcyxhw,ocyx->bhwo", t, w) + b32.astype(np.float64)
    mag = np.einsum("bcyxhw,ocyx->bhwo", np.abs(t), np.abs(w)) + np.abs(b32.astype(np.float64))
    return pre / (1.0 + np.exp(-pre)), mag


def stem6_bound(ref, mag):
    return 2.0 ** -11 * np.abs(ref) + 1.1 * 128 * U * mag + 2.0 ** -21 * np.abs(ref)


def stem6_f32_cpu(x16, w16, b32, mut=None):
    """The kernel in float32: products of fp16 values are exact, summed in fp32 in K order (c, ky, kx), + bias, fast-exp SiLU, one
    rounding to fp16.  ``mut``: ``tap_shift`` (tap (c=1, ky=2, kx=3) reads one pixel further right), ``pad3`` (padding 3)."""
    assert mut in (None,) + STEM_MUTANTS
    B, _, H, W = x16.shape
    t = _taps(x16.astype(np.float32), H // 2, W // 2, 3 if mut == "pad3" else 2, np.float32)
    if mut == "tap_shift":
        t[:, 1, 2, 3] = t[:, 1, 2, 4]
    w = w16.astype(np.float32)
    acc = np.zeros((B, H // 2, W // 2, w.shape[0]), dtype=np.float32)
    for c in range(3):
        for ky in range(6):
            for kx in range(6):
                acc += t[:, c, ky, kx][..., None] * w[:, c, ky, kx]
    v = acc + b32.astype(np.float32)
    return (v * _fast_sigmoid32(v)).astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------ head
def logits_f64(x16, w16, b32):
    """``x16`` [B,h,w,Cin] fp16, ``w16`` [Cout,Cin] fp16, ``b32`` [Cout] -> (z, mag) [B,h,w,Cout] float64."""
    x, w = x16.astype(np.float64), w16.astype(np.float64)
    return x @ w.T + b32.astype(np.float64), np.abs(x) @ np.abs(w).T + np.abs(b32.astype(np.float64))


def head5_decode(z, anchors_lv, stride, nc, mut=None, other_lv=None, sigmoid=None):
    """``z`` [B,h,w,3*(5+nc)] logits -> [B, 5+nc, 3*h*w] in ``z``'s dtype, anchor index a*h*w + y*w + x.  ``anchors_lv`` [3,2]."""
    assert mut in (None,) + HEAD_MUTANTS
    B, h, w, _ = z.shape
    no, dt = 5 + nc, z.dtype
    y = (1.0 / (1.0 + np.exp(-z))) if sigmoid is None else sigmoid(z)
    y = y.reshape(B, h, w, 3, no).astype(dt)
    gx = np.arange(w, dtype=dt).reshape(1, 1, w, 1)
    gy = np.arange(h, dtype=dt).reshape(1, h, 1, 1)
    if mut == "swap_xy":
        gx, gy = gy, gx
    off = dt.type(0.0 if mut == "grid_zero" else 0.5)
    anc = np.asarray(other_lv if mut == "wrong_level" else anchors_lv).astype(dt).reshape(1, 1, 1, 3, 2)
    out = y.copy()
    out[..., 0] = (y[..., 0] * dt.type(2) - off + gx) * dt.type(stride)
    out[..., 1] = (y[..., 1] * dt.type(2) - off + gy) * dt.type(stride)
    t = y[..., 2:4] * dt.type(2)
    out[..., 2:4] = (t if mut == "no_square" else t * t) * anc
    return np.ascontiguousarray(out.transpose(0, 4, 3, 1, 2)).reshape(B, no, 3 * h * w)


def head5_bound(z, mag, cin, anchors_lv, stride, nc, staged_f16=True):
    """(bound for the fp16 head [B, 5+nc, 3hw], bound for boxes32 [B, 4, 3hw], float64 reference)."""
    B, h, w, _ = z.shape
    no = 5 + nc
    ref = head5_decode(z, anchors_lv, stride, nc)
    dz = cin * U * mag + (2.0 ** -11 * np.abs(z) if staged_f16 else 0.0)
    y = 1.0 / (1.0 + np.exp(-z))
    dy = (y * (1.0 - y)).reshape(B, h, w, 3, no)
    yv = y.reshape(B, h, w, 3, no)
    der = dy.copy()
    der[..., 0:2] = 2.0 * stride * dy[..., 0:2]
    der[..., 2:4] = 8.0 * yv[..., 2:4] * dy[..., 2:4] * np.asarray(anchors_lv, dtype=np.float64).reshape(1, 1, 1, 3, 2)
    err = der * dz.reshape(B, h, w, 3, no)
    err = np.ascontiguousarray(err.transpose(0, 4, 3, 1, 2)).reshape(B, no, 3 * h * w)
    return err + ulp16(ref) / 2, err[:, :4] + 2.0 ** -22 * np.abs(ref[:, :4]), ref


def head5_f32_cpu(x16, w16, b32, anchors_lv, stride, nc, mut=None, other_lv=None):
    """The kernel in float32: fp32 logit (summation order aside), rounded to fp16, fast sigmoid, the decode in the kernel's order,
    one rounding to fp16.  Returns (head fp16 [B, 5+nc, 3hw], boxes32 fp32 [B, 4, 3hw])."""
    z = (x16.astype(np.float32) @ w16.astype(np.float32).T + b32.astype(np.float32)).astype(np.float16).astype(np.float32)
    out = head5_decode(z, anchors_lv, stride, nc, mut=mut, other_lv=other_lv, sigmoid=_fast_sigmoid32)
    return out.astype(np.float16), out[:, :4].copy()
