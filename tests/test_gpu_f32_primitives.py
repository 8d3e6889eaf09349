"""The fp32 plan's non-convolution primitives on their own, through the C ABI: rva_maxpool5_nhwc_f32 and rva_upsample2x_nhwc_f32
(exact), rva_stem_conv_f32 against a float64 convolution + SiLU.  Every call reads and writes a channel slice of a wider row
(ldi, ldo > C at a channel offset); whatever lies outside the written slice must still hold the sentinel.

Pools run twice, once on all-negative input drawn from [-3, -1]: a pool that pads with 0 instead of -inf is then wrong at every
border pixel (on zero-mean input it is wrong only where a whole clipped window is negative).  (2,3,2,8): every window is clipped on
all four sides.

Stem bound (tests/clip_stage_refs.py): the 27-term dot product plus bias errs by (27 + 2) u (conv(|x|, |w|) + |b|); SiLU carries
it with |silu'| <= 1.1 and adds 4 u |ref| for expf, the addition and the division."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops
from tests import clip_stage_refs as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
# (B, H, W, C, ldi, input channel offset)
POOL_SHAPES = [(2, 20, 20, 32, 96, 64), (3, 13, 17, 4, 12, 4), (1, 1, 1, 4, 12, 4), (2, 3, 2, 8, 16, 4)]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _input(shape, negative, seed):
    g = torch.Generator().manual_seed(seed)
    return -(torch.rand(shape, generator=g) * 2 + 1) if negative else torch.randn(shape, generator=g)


def _slice_ok(out, off, C_, want, what):
    assert torch.equal(out[..., off:off + C_], want), what
    outside = torch.ones(out.shape[-1], dtype=torch.bool)
    outside[off:off + C_] = False
    assert bool((out[..., outside] == SENTINEL).all()), (what, "written outside the channel slice")


@pytest.mark.parametrize("negative", [False, True], ids=["zero-mean", "all-negative"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
def test_maxpool5_and_upsample2x_f32_are_exact(shape, negative):
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, H, W, C_, ldi, off = shape
    ldo, ooff = C_ + 12, 8
    row = _input((B, H, W, ldi), negative, 31)
    x = row[..., off:off + C_].contiguous()
    if negative:
        assert float(x.max()) <= -1.0 and float(x.min()) >= -3.0
    dev = row.cuda()
    out = torch.full((B, H, W, ldo), SENTINEL, device="cuda")
    ctx.check(L.rva_maxpool5_nhwc_f32(ctx.handle, _ptr(dev, off), ldi, _ptr(out, ooff), ldo, B, H, W, C_, s), "rva_maxpool5_nhwc_f32")
    up = torch.full((B, 2 * H, 2 * W, ldo), SENTINEL, device="cuda")
    ctx.check(L.rva_upsample2x_nhwc_f32(ctx.handle, _ptr(dev, off), ldi, _ptr(up, ooff), ldo, B, H, W, C_, s), "rva_upsample2x_nhwc_f32")
    torch.cuda.synchronize()
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1)
    if negative:
        assert float(want.max()) <= -1.0                              # a zero-padded pool would return 0 at every border pixel
    _slice_ok(out.cpu(), ooff, C_, want, "maxpool5")
    _slice_ok(up.cpu(), ooff, C_, x.repeat_interleave(2, 1).repeat_interleave(2, 2), "upsample2x")


@pytest.mark.parametrize("Cout", [16, 48])
@pytest.mark.parametrize("shape", [(2, 9, 7), (1, 16, 24), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_stem_conv_f32_against_float64(shape, Cout):
    L, ctx, s = N.lib(), ops.context(), _stream()
    B, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(41 + Cout)
    x = torch.randn((B, 3, H, W), generator=g)
    w = torch.randn((Cout, 3, 3, 3), generator=g) * 0.4                # [Cout][c][ky][kx]: the 27 taps in the kernel's order
    b = torch.randn((Cout,), generator=g) * 0.5
    ldo, off = Cout + 8, 4
    out = torch.full((B, Ho, Wo, ldo), SENTINEL, device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    ctx.check(L.rva_stem_conv_f32(ctx.handle, _ptr(xd), _ptr(wd), _ptr(bd), _ptr(out, off), ldo, B, H, W, Cout, s), "rva_stem_conv_f32")
    torch.cuda.synchronize()
    out = out.cpu()
    y, tol_y = R.conv_bound(F.conv2d, x, w, b, 27, stride=2, padding=1)
    ref = F.silu(y)
    tol = 1.1 * tol_y + 4 * R.U * ref.abs()
    assert tuple(ref.shape) == (B, Cout, Ho, Wo)
    got = out[..., off:off + Cout].permute(0, 3, 1, 2)
    bad = []
    R.report(shape + (Cout,), "rva_stem_conv_f32", got, ref, tol, out=bad)
    assert not bad, bad
    outside = torch.ones(ldo, dtype=torch.bool)
    outside[off:off + Cout] = False
    assert bool((out[..., outside] == SENTINEL).all())
