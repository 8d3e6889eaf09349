"""The two YOLO11 kernels on the GPU against the float64 references and bounds of tests/yolo11_refs.py: ``rva_dwconv3x3_nhwc_f16``
and ``rva_psa_attention_f16``.  Inputs and outputs are channel slices of wider buffers whose other channels hold a sentinel that
must survive; observed / bound is printed per case.  Bit-identity: image 0 of a batch of two == the image alone; a hipGraph replay
== the eager launch.  Every refused argument is a ``RuntimeError`` naming the entry, and nothing is launched (the output keeps its
sentinel)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from tests import yolo11_refs as R

pytestmark = pytest.mark.gpu

SENTINEL = -1234.0


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------ depthwise
@functools.lru_cache(maxsize=None)
def _dw_data(C_, H, W, B=2):
    rng = np.random.default_rng(1000 * C_ + 10 * H + W)
    x = rng.normal(0, 1.5, (B, H, W, C_)).astype(np.float16)
    w = rng.normal(0, 0.5, (C_, 3, 3)).astype(np.float16)
    b = rng.normal(0, 0.5, C_).astype(np.float32)
    r = rng.normal(0, 2.0, (B, H, W, C_)).astype(np.float16)
    return x, w, b, r


def _dw_buffers(x, r, C_):
    """x in channels [8, 8 + C) of a buffer of C + 16, the residual in [16, 16 + C) of C + 24, out in [24, 24 + C) of C + 32."""
    B, H, W, _ = x.shape
    xin = torch.full((B, H, W, C_ + 16), SENTINEL, dtype=torch.float16, device="cuda")
    xin[..., 8:8 + C_] = torch.from_numpy(x).cuda()
    res = torch.full((B, H, W, C_ + 24), SENTINEL, dtype=torch.float16, device="cuda")
    res[..., 16:16 + C_] = torch.from_numpy(r).cuda()
    out = torch.full((B, H, W, C_ + 32), SENTINEL, dtype=torch.float16, device="cuda")
    return xin, res, out


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7), (20, 20)])
@pytest.mark.parametrize("C_", [8, 64, 80, 136])
def test_depthwise_against_float64(C_, hw):
    x, w, b, r = _dw_data(C_, *hw)
    wp = ops.pack_dwconv_weights(torch.from_numpy(w.astype(np.float32))[:, None]).cuda()
    assert torch.equal(wp.cpu(), torch.from_numpy(w).reshape(C_, 9).t())
    bias = torch.from_numpy(b).cuda()
    bad = []
    for act in (0, 1):
        for with_res in (False, True):
            xin, res, out = _dw_buffers(x, r, C_)
            ops.dwconv3x3_f16(xin[..., 8:8 + C_], wp, bias, out[..., 24:24 + C_], act=bool(act),
                              residual=res[..., 16:16 + C_] if with_res else None)
            torch.cuda.synchronize()
            ref, pre, mag = R.dw_f64(x, w, b, act, r if with_res else None)
            R.check(f"dwconv C {C_} {hw[0]}x{hw[1]}", f"act {act} residual {with_res}", out[..., 24:24 + C_].cpu().numpy(), ref,
                    R.dw_bound(ref, pre, mag, act, with_res), bad)
            assert bool((out[..., :24] == SENTINEL).all()) and bool((out[..., 24 + C_:] == SENTINEL).all()), "wrote outside its slice"
            assert bool((xin[..., :8] == SENTINEL).all()) and bool((xin[..., 8 + C_:] == SENTINEL).all())
    assert not bad, bad


def test_depthwise_batch_independence_and_graph_replay():
    C_, hw = 80, (5, 7)
    x, w, b, r = _dw_data(C_, *hw)
    wp = ops.pack_dwconv_weights(torch.from_numpy(w.astype(np.float32))[:, None]).cuda()
    bias = torch.from_numpy(b).cuda()
    xin, res, out = _dw_buffers(x, r, C_)
    args = dict(act=True, residual=res[..., 16:16 + C_])
    both = ops.dwconv3x3_f16(xin[..., 8:8 + C_], wp, bias, out[..., 24:24 + C_], **args).clone()
    out.fill_(SENTINEL)
    one = ops.dwconv3x3_f16(xin[:1, ..., 8:8 + C_], wp, bias, out[:1, ..., 24:24 + C_], act=True, residual=res[:1, ..., 16:16 + C_])
    torch.cuda.synchronize()
    assert torch.equal(_bits(one), _bits(both[:1])) and bool((out[1] == SENTINEL).all())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops.dwconv3x3_f16(xin[..., 8:8 + C_], wp, bias, out[..., 24:24 + C_], **args)
    out.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[..., 24:24 + C_]), _bits(both))


# ------------------------------------------------------------------------------------------------------------ attention
def _attn_buffers(qkv, heads):
    """qkv in channels [8, 8 + 128 heads) of a buffer of 128 heads + 16, out in [8, 8 + 64 heads) of 64 heads + 16."""
    B, T, _ = qkv.shape
    buf = torch.full((B, T, 128 * heads + 16), SENTINEL, dtype=torch.float16, device="cuda")
    buf[..., 8:8 + 128 * heads] = torch.from_numpy(qkv).cuda()
    out = torch.full((B, T, 64 * heads + 16), SENTINEL, dtype=torch.float16, device="cuda")
    return buf, out


@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("tokens", [1, 6, 20, 33, 110, 400])
def test_attention_against_float64(tokens, heads):
    bad = []
    for kind in ("uniform", "peaked", "tied"):
        qkv = R.attn_inputs(kind, 2, tokens, heads, 128 * heads, seed=tokens + heads)
        buf, out = _attn_buffers(qkv, heads)
        ops.psa_attention_f16(buf[..., 8:8 + 128 * heads], out[..., 8:8 + 64 * heads], heads)
        torch.cuda.synchronize()
        ref, tol = R.attn_f64(qkv, heads)
        got = out[..., 8:8 + 64 * heads].cpu().numpy()
        R.check(f"attention T {tokens} heads {heads}", kind, got, ref, tol, bad)
        assert bool((out[..., :8] == SENTINEL).all()) and bool((out[..., 8 + 64 * heads:] == SENTINEL).all()), "wrote outside its slice"
        if kind == "tied":                                                 # every key equal: the mean of v, within the same bound
            v = qkv.astype(np.float64).reshape(2, tokens, heads, 128)[..., 64:]
            mean = np.broadcast_to(v.mean(1, keepdims=True), v.shape).reshape(2, tokens, 64 * heads)
            R.check(f"attention T {tokens} heads {heads}", "tied against the mean of v", got, mean, tol, bad)
    assert not bad, bad


def test_attention_batch_independence_and_graph_replay():
    tokens, heads = 110, 2
    qkv = R.attn_inputs("uniform", 2, tokens, heads, 128 * heads, seed=9)
    buf, out = _attn_buffers(qkv, heads)
    both = ops.psa_attention_f16(buf[..., 8:8 + 128 * heads], out[..., 8:8 + 64 * heads], heads).clone()
    out.fill_(SENTINEL)
    one = ops.psa_attention_f16(buf[:1, :, 8:8 + 128 * heads], out[:1, :, 8:8 + 64 * heads], heads)
    torch.cuda.synchronize()
    assert torch.equal(_bits(one), _bits(both[:1])) and bool((out[1] == SENTINEL).all())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops.psa_attention_f16(buf[..., 8:8 + 128 * heads], out[..., 8:8 + 64 * heads], heads)
    out.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[..., 8:8 + 64 * heads]), _bits(both))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refused_arguments_launch_nothing():
    ctx, L = ops.context(), N.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros((1, 4, 4, 32), dtype=torch.float16, device="cuda")
    out = torch.full((1, 4, 4, 32), SENTINEL, dtype=torch.float16, device="cuda")
    w = torch.zeros((9, 32), dtype=torch.float16, device="cuda")
    b = torch.zeros(32, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                    # noqa: E731

    def dw(xin=p(x), ldi=32, wt=p(w), bias=p(b), o=p(out), ldo=32, res=None, ldr=0, batch=1, H=4, W=4, ch=16, act=1):
        return L.rva_dwconv3x3_nhwc_f16(ctx.handle, xin, ldi, wt, bias, o, ldo, res, ldr, batch, H, W, ch, act, st)
    assert dw() == N.RVA_OK
    torch.cuda.synchronize()
    assert bool((out[..., :16] == 0).all()) and bool((out[..., 16:] == SENTINEL).all())
    out.fill_(SENTINEL)
    refused = dict(c_not_8=dict(ch=12), c_zero=dict(ch=0), ldi_small=dict(ldi=8), ldo_small=dict(ldo=8), ldr_small=dict(res=p(x), ldr=8),
                   in_misaligned=dict(xin=p(x, 2)), out_misaligned=dict(o=p(out, 8)), w_misaligned=dict(wt=p(w, 4)),
                   res_misaligned=dict(res=p(x, 6), ldr=32), batch_zero=dict(batch=0), h_zero=dict(H=0), w_negative=dict(W=-1),
                   no_input=dict(xin=None), no_bias=dict(bias=None))
    for name, kw in refused.items():
        rc = dw(**kw)
        assert rc == N.RVA_ERR_ARG, name
        with pytest.raises(RuntimeError, match="rva_dwconv3x3_nhwc_f16: batch, H, W > 0"):
            ctx.check(rc, name)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call launched"

    q = torch.zeros((1, 8, 256), dtype=torch.float16, device="cuda")
    o2 = torch.full((1, 8, 128), SENTINEL, dtype=torch.float16, device="cuda")

    def at(qkv=p(q), ld=256, o=p(o2), ldo=128, batch=1, tokens=8, heads=2):
        return L.rva_psa_attention_f16(ctx.handle, qkv, ld, o, ldo, batch, tokens, heads, st)
    assert at() == N.RVA_OK
    torch.cuda.synchronize()
    assert bool((o2 == 0).all())                                            # v = 0: the mean of v
    o2.fill_(SENTINEL)
    refused = dict(heads_zero=dict(heads=0), ld_small=dict(ld=248), ldo_small=dict(ldo=120), tokens_zero=dict(tokens=0),
                   batch_zero=dict(batch=0), qkv_misaligned=dict(qkv=p(q, 8)), out_misaligned=dict(o=p(o2, 2)), heads_3_of_2=dict(heads=3),
                   no_output=dict(o=None))
    for name, kw in refused.items():
        rc = at(**kw)
        assert rc == N.RVA_ERR_ARG, name
        with pytest.raises(RuntimeError, match="rva_psa_attention_f16: batch, tokens, heads >= 1"):
            ctx.check(rc, name)
    torch.cuda.synchronize()
    assert bool((o2 == SENTINEL).all()), "a refused call launched"
    # through the wrappers a refusal is a RuntimeError naming the entry
    with pytest.raises(RuntimeError, match="rva_dwconv3x3_nhwc_f16"):
        ops.dwconv3x3_f16(x[..., :12], w[:, :12].contiguous(), b[:12].contiguous(), out[..., :12])
    with pytest.raises(RuntimeError, match="rva_psa_attention_f16"):
        ops.psa_attention_f16(q[..., 4:], o2, 1)
