"""CPU-only proof that the stage bounds of tests/resnet_stage_refs.py can see the bugs k_res_conv and k_res_mean can make, and
that a correct fp32 implementation meets them.

torch's own fp32 operators on the CPU, fed the fp32 taps, must stay inside every bound at the four shapes; and each bug class,
applied to the float64 reference, must leave its stage's bound by a factor of at least 4 at one element or more on at least
one of the shapes (the rule of tests/test_clip_stages_host.py).  The "taps" are the float64 references rounded once to fp32."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import resnet_stage_refs as R

FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def _case(shape):
    net, p, frames = R.case(shape)
    refs = R.refs(None, frames, p, shape)
    return p, frames, refs, {k: v[0].float() for k, v in refs.items()}


def _block_in(taps, b):
    return taps["pooled" if b == 0 else f"out{b - 1}"]


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_torch_fp32_is_inside_every_bound(shape):
    p, frames, refs, taps = _case(shape)
    q = {k: v.float() for k, v in p.items()}
    got = {}
    y = F.conv2d(frames.float(), q["stem_w"], q["stem_b"], stride=2, padding=3)
    got["pooled"] = F.max_pool2d(y.relu(), 3, 2, 1).permute(0, 2, 3, 1)
    alive = {}
    for b, (cin, c, s) in enumerate(R.BLOCKS):
        x = _block_in(taps, b).permute(0, 3, 1, 2)
        i = R.CONV_OF[f"mid{b}"]
        got[f"mid{b}"] = F.conv2d(x, q[f"c{i}_w"], q[f"c{i}_b"], stride=s, padding=1).relu().permute(0, 2, 3, 1)
        r = x
        if b in R.DOWN:
            i = R.CONV_OF[f"down{b}"]
            got[f"down{b}"] = F.conv2d(x, q[f"c{i}_w"], q[f"c{i}_b"], stride=2).permute(0, 2, 3, 1)
            r = taps[f"down{b}"].permute(0, 3, 1, 2)
        i = R.CONV_OF[f"out{b}"]
        y = F.conv2d(taps[f"mid{b}"].permute(0, 3, 1, 2), q[f"c{i}_w"], q[f"c{i}_b"], padding=1)
        got[f"out{b}"] = ((y + r).relu()).permute(0, 2, 3, 1)
        alive[b] = (float((taps[f"mid{b}"] > 0).float().mean()), float((taps[f"out{b}"] > 0).float().mean()))
    v = taps["out7"].flatten(1, 2)
    got["feat"] = v.sum(1) / torch.tensor(float(v.shape[1]), dtype=torch.float32)
    got["logits"] = taps["feat"] @ q["head_w"].T + q["head_b"]
    print(f"{R.shape_id(shape)}: ReLUs alive (mid, out) per block: " + ", ".join(f"{a:.2f}/{o:.2f}" for a, o in alive.values()))
    assert all(0.05 < a < 1.0 and 0.05 < o <= 1.0 for a, o in alive.values())     # no stage is trivially zero
    bad = []
    for k, t in got.items():
        assert t.dtype == torch.float32
        R.report(shape, k, t, *refs[k], out=bad)
    assert not bad, bad


def _worst(mutate, stages):
    """max over the shapes and the given stages of (the mutation's distance from the reference / bound); ``mutate(shape, name)``
    returns the mutated float64 stage in the tap layout or None where the shape cannot show the bug."""
    seen = {}
    for shape in R.SHAPES:
        _, _, refs, _ = _case(shape)
        for name in stages:
            m = mutate(shape, name)
            if m is not None:
                seen[(R.shape_id(shape), name)] = R.ratio(m, *refs[name])[0]
    print({k: round(v, 1) for k, v in seen.items()})
    return max(seen.values())


def _conv(shape, name, x=None, w_kw=None, bias=None):
    p, _, _, taps = _case(shape)
    b = int(name[-1])
    i = R.CONV_OF[name]
    x = R.nchw(_block_in(taps, b) if not name.startswith("out") else taps[f"mid{b}"]) if x is None else x
    q = dict(p)
    if bias is not None:
        q[f"c{i}_b"] = bias(p[f"c{i}_b"])
    return R.block_conv(name, x, q, **(w_kw or {}))[0]


def _shortcut(shape, b):
    _, _, _, taps = _case(shape)
    return R.nchw(taps[f"down{b}"] if b in R.DOWN else _block_in(taps, b))


def test_stride2_origin_off_by_one_is_seen():
    def mutate(shape, name):
        _, _, _, taps = _case(shape)
        x = R.nchw(_block_in(taps, int(name[-1])))
        shifted = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]                      # input row 2 oy + ky - pad + 1
        y = _conv(shape, name, x=shifted)
        return R.nhwc(y.relu() if name.startswith("mid") else y)
    assert _worst(mutate, ("mid2", "down2", "mid4", "down4", "mid6", "down6")) > FACTOR


@pytest.mark.parametrize("bug", ["after_relu", "dropped"])
def test_residual_in_the_wrong_place_is_seen(bug):
    def mutate(shape, name):
        b = int(name[-1])
        y = _conv(shape, name)
        return R.nhwc(y.relu() + _shortcut(shape, b) if bug == "after_relu" else y.relu())
    assert _worst(mutate, tuple(f"out{b}" for b in range(8))) > FACTOR


def test_pixel_to_image_decomposition_wrong_at_an_image_boundary_is_seen():
    """The rows of a 32-row tile that lie past an image boundary take the tile's first row's image: they hold the previous
    image's pixel of the same (y, x)."""
    def mutate(shape, name):
        _, _, refs, _ = _case(shape)
        ref = refs[name][0]
        B, h, w, c = ref.shape
        P = h * w
        if B < 2 or P % 32 == 0:
            return None
        flat = ref.reshape(B * P, c).clone()
        for img in range(1, B):
            lo = img * P
            hi = min(-(-lo // 32) * 32, B * P)
            if lo % 32:
                flat[lo:hi] = ref.reshape(B * P, c)[lo - P:hi - P]
        return flat.view(B, h, w, c)
    assert _worst(mutate, ("mid0", "out0", "down2", "out7")) > FACTOR


def test_shortcut_taken_with_pad_1_is_seen():
    def mutate(shape, name):
        _, _, refs, _ = _case(shape)
        y = _conv(shape, name, w_kw={"padding": 1})                          # input row 2 oy - 1
        h, w = refs[name][0].shape[1:3]
        return R.nhwc(y[:, :, :h, :w])
    assert _worst(mutate, ("down2", "down4", "down6")) > FACTOR


def test_another_channels_bias_is_seen():
    def mutate(shape, name):
        y = _conv(shape, name, bias=lambda b: b.roll(1))
        if name.startswith("out"):
            return R.nhwc((y + _shortcut(shape, int(name[-1]))).relu())
        return R.nhwc(y.relu() if name.startswith("mid") else y)
    for stages in (("mid0", "mid5"), ("down2", "down6"), ("out1", "out6")):
        assert _worst(mutate, stages) > FACTOR


def test_last_pixel_missing_from_the_mean_is_seen():
    def mutate(shape, name):
        _, _, _, taps = _case(shape)
        v = R.f64(taps["out7"]).flatten(1, 2)
        return None if v.shape[1] < 2 else v[:, :-1].sum(1) / v.shape[1]
    assert _worst(mutate, ("feat",)) > FACTOR
