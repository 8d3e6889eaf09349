"""References, fp32 restatements and bounds for the two YOLO11 kernels (``rva_dwconv3x3_nhwc_f16``, ``rva_psa_attention_f16``),
shared by tests/test_yolo11_host.py (CPU: the restatements stay inside the bounds, planted errors leave them) and
tests/test_gpu_yolo11_prims.py.  ``U = 2^-24`` is the unit roundoff of fp32.  Nothing is fitted to a kernel's output.

Depthwise: ``dw_f64`` is the float64 result from the fp16 inputs and weights, with ``pre`` (before SiLU) and ``mag = sum |x w| +
|b|`` per output.  The kernel adds nine products, each exact in fp32, and the bias: nine roundings of partial sums no larger than
``mag``.  SiLU' <= 1.1; the fast SiLU (``v * rcp(1 + exp2(-v log2 e))``) is good to ``(2 + |pre|) 2^-22`` relative; the residual add
rounds once in fp32; the result is rounded once to fp16:
    ulp16(ref) / 2 + s * 9 U mag + [act] (2 + |pre|) 2^-22 |silu(pre)| + [res] U |ref|,   s = 1.1 with SiLU, else 1.

Attention, per (image, head, query): ``S_k = scale * q . k_k``, ``w_k = softmax_k(S)``, ``ref_d = sum_k w_k v_kd``.
  1. fp32 rounding of S: 32 exact products summed in fp32 and one multiplication by the rounded scale:
     ``dS_k = 33 U scale sum_i |q_i k_ki| + 2 U |S_k|``.  The exponent ``a_k = S_k - m`` is rounded (U |a_k|), multiplied by log2 e
     (U |a_k|) and exponentiated (2^-22): the relative error of p_k is  e_k = dS_k + 2 U |a_k| + 2^-22  (the maximum m and the
     rescaling of the online softmax are common factors of the numerator and the row sum).  To first order a relative error e_k of
     p_k moves the result by at most  sum_k w_k |v_kd| e_k + (sum_k w_k e_k) W_d,  W_d = sum_k w_k |v_kd|.
  2. fp16 rounding of P: 2^-11 relative per entry, weighted by |V|: ``2^-11 W_d``; an entry below 2^-14 is subnormal in fp16 and
     off by up to 2^-25 absolute, against a row sum >= 1: ``2^-25 sum_k |v_kd| / sum_k p_k``.
  3. fp32 sums: the row sum and the accumulator take T terms each (``2 T U W_d``), every key tile rescales both
     (``4 tiles U W_d``), the division rounds (``8 U W_d`` with slack).
  4. the final half ulp of fp16.
``attn_f32_cpu`` restates the kernel in numpy float32 with the same rounding points (online over key tiles of 32, P rounded to
fp16, ``__expf`` as float32 exp2 of float32(x * float32(log2 e))) and takes ``mut=``: ``no_max`` (no maximum subtracted) or
``scale_twice`` (S scaled by 32^-0.5 twice)."""
import numpy as np

U = 2.0 ** -24
LOG2E32 = np.float32(1.4426950408889634)
SCALE = 32.0 ** -0.5
SCALE32 = np.float32(0.17677669529663687)
ATTN_MUTANTS = ("no_max", "scale_twice")
DW_MUTANTS = ("tap_swap", "no_pad")


def ulp16(v):
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def check(entry, what, got, ref, tol, bad):
    """max |got - ref| / tol over all elements, printed; a ratio above 1 (or a non-finite ``got``) is appended to ``bad``."""
    got, ref, tol = (np.asarray(v, dtype=np.float64) for v in (got, ref, tol))
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / tol)
    r = float(np.nanmax(ratio)) if np.isfinite(got).all() else float("inf")
    worst = float(np.nanmax(err)) if np.isfinite(err).any() else float("nan")
    print(f"[{entry}] {what}: max |d| {worst:.4g}, max observed / bound {r:.3f}")
    if not r <= 1.0:
        bad.append((entry, what, r))
    return r


def _fast_exp32(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp2((x.astype(np.float32) * LOG2E32).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ depthwise
def _dw_taps(x, dtype, pad=True):
    """``[3, 3, B, H, W, C]``: tap (ky, kx) of every output, zero outside the image (``pad=False``: edge replicated)."""
    B, H, W, C = x.shape
    xp = np.pad(x.astype(dtype), ((0, 0), (1, 1), (1, 1), (0, 0)), mode="constant" if pad else "edge")
    return np.stack([np.stack([xp[:, ky:ky + H, kx:kx + W] for kx in range(3)]) for ky in range(3)])


def dw_f64(x16, w16, b32, act, res16=None):
    """``x16`` [B,H,W,C] fp16, ``w16`` [C,3,3] fp16, ``b32`` [C] fp32 -> (ref, pre, mag), each [B,H,W,C] float64."""
    t = _dw_taps(x16, np.float64)
    w = w16.astype(np.float64).transpose(1, 2, 0)[:, :, None, None, None, :]
    b = b32.astype(np.float64)
    pre = (t * w).sum((0, 1)) + b
    mag = np.abs(t * w).sum((0, 1)) + np.abs(b)
    ref = pre / (1.0 + np.exp(-pre)) if act else pre.copy()
    if res16 is not None:
        ref = ref + res16.astype(np.float64)
    return ref, pre, mag


def dw_bound(ref, pre, mag, act, has_res):
    tol = ulp16(ref) / 2 + (1.1 if act else 1.0) * 9 * U * mag
    if act:
        tol = tol + (2.0 + np.abs(pre)) * 2.0 ** -22 * np.abs(pre / (1.0 + np.exp(-pre)))
    if has_res:
        tol = tol + U * np.abs(ref)
    return tol


def dw_f32_cpu(x16, w16, b32, act, res16=None, mut=None):
    """The kernel in float32: the nine products added from zero in (ky, kx) order, bias, fast SiLU, residual, one rounding."""
    assert mut in (None,) + DW_MUTANTS
    t = _dw_taps(x16, np.float32, pad=mut != "no_pad")
    w = w16.astype(np.float32)
    if mut == "tap_swap":
        w = w.transpose(0, 2, 1)
    acc = np.zeros(x16.shape, dtype=np.float32)
    for ky in range(3):
        for kx in range(3):
            acc = (acc + t[ky, kx] * w[:, ky, kx]).astype(np.float32)
    v = (acc + b32.astype(np.float32)).astype(np.float32)
    if act:
        v = (v * (np.float32(1.0) / (np.float32(1.0) + _fast_exp32(-v)))).astype(np.float32)
    if res16 is not None:
        v = (v + res16.astype(np.float32)).astype(np.float32)
    return v.astype(np.float16)


# ------------------------------------------------------------------------------------------------------------ attention
def attn_inputs(kind, B, T, heads, ld, seed=0):
    """fp16 ``[B, T, ld]`` with ``ld >= 128 heads``; the channels behind the heads hold a sentinel (they are never read).
    ``uniform``: everything N(0, 1).  ``peaked``: q and k scaled so that the logits of a row span more than 88 (exp overflows in
    fp32 without the maximum subtracted).  ``tied``: every key equal (q and v random): the result is the mean of v."""
    assert kind in ("uniform", "peaked", "tied") and ld >= 128 * heads
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (B, T, ld))
    x[:, :, 128 * heads:] = 777.0
    for h in range(heads):
        q, k = slice(128 * h, 128 * h + 32), slice(128 * h + 32, 128 * h + 64)
        if kind == "peaked":
            x[:, :, q] = np.sign(x[:, :, q]) * 6.0
            x[:, :, k] = np.sign(x[:, :, k]) * 6.0 * rng.uniform(0.5, 1.0, (B, T, 1))
            x[:, 0, k] = x[:, 0, q] * 1.0                  # key 0 is aligned with query 0: logit 32 * 36 * scale = 203
        elif kind == "tied":
            x[:, :, k] = x[:, :1, k]
    return x.astype(np.float16)


def _split(qkv16, heads, dtype):
    B, T, _ = qkv16.shape
    x = qkv16[:, :, :128 * heads].astype(dtype).reshape(B, T, heads, 128).transpose(0, 2, 1, 3)      # [B, heads, T, 128]
    return x[..., :32], x[..., 32:64], x[..., 64:]


def attn_f64(qkv16, heads):
    """-> (ref, tol), both ``[B, T, 64 heads]`` float64: the module's attention on the fp16 inputs, and the bound of this file's
    docstring around it."""
    B, T, _ = qkv16.shape
    q, k, v = _split(qkv16, heads, np.float64)
    S = SCALE * (q @ k.transpose(0, 1, 3, 2))
    magS = SCALE * (np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2))
    a = S - S.max(-1, keepdims=True)
    p = np.exp(a)
    L = p.sum(-1, keepdims=True)
    w = p / L
    ref = w @ v
    e = 33 * U * magS + 2 * U * np.abs(S) + 2 * U * np.abs(a) + 2.0 ** -22
    W = w @ np.abs(v)
    tiles = (T + 31) // 32
    tol = (w * e) @ np.abs(v) + (w * e).sum(-1, keepdims=True) * W          # 1. S and the exponential
    tol += 2.0 ** -11 * W + 2.0 ** -25 * np.abs(v).sum(-2, keepdims=True) / L   # 2. P in fp16
    tol += (2 * T + 4 * tiles + 8) * U * W                                   # 3. fp32 sums, rescaling, division
    tol += ulp16(ref) / 2                                                    # 4. the result in fp16
    back = lambda t: t.transpose(0, 2, 1, 3).reshape(B, T, 64 * heads)      # noqa: E731
    return back(ref), back(tol)


def attn_f32_cpu(qkv16, heads, mut=None):
    """The kernel in float32, ``[B, T, 64 heads]`` fp16."""
    assert mut in (None,) + ATTN_MUTANTS
    B, T, _ = qkv16.shape
    q, k, v = _split(qkv16, heads, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        S = ((q @ k.transpose(0, 1, 3, 2)).astype(np.float32) * SCALE32).astype(np.float32)
        if mut == "scale_twice":
            S = (S * SCALE32).astype(np.float32)
        m = np.full((B, heads, T, 1), -np.inf, dtype=np.float32)
        l = np.zeros((B, heads, T, 1), dtype=np.float32)
        o = np.zeros((B, heads, T, 64), dtype=np.float32)
        for k0 in range(0, T, 32):
            s = S[..., k0:k0 + 32]
            mn = np.maximum(m, s.max(-1, keepdims=True))
            if mut == "no_max":
                mn = np.zeros_like(mn)
            alpha = _fast_exp32(m - mn) if mut != "no_max" else np.ones_like(mn)
            p = _fast_exp32((s - mn).astype(np.float32))
            l = (l * alpha + p.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
            o = (o * alpha + (p.astype(np.float16).astype(np.float32) @ v[:, :, k0:k0 + 32]).astype(np.float32)).astype(np.float32)
            m = mn
        out = (o / l).astype(np.float32)
    return out.transpose(0, 2, 1, 3).reshape(B, T, 64 * heads).astype(np.float16)
