"""CPU-only proof that the bounds of tests/head_refs.py can see the mistakes a detect-head kernel can make, and that a correct
fp32 implementation meets them.

  * ``head_ref`` is ``yolov8.DetectHead.forward``: a float64 ``YoloV8`` on its own raw logits, to 1e-12 relative.
  * ``head_f32_cpu`` -- the kernels restated in float32, in both exp forms -- stays inside the bounds on every logit set and geometry
    of tests/test_gpu_head_f64.py (observed / bound is printed: ``pytest -s``).  The derivation of the bounds needed no correction.
  * every mutant of ``head_f32_cpu`` leaves the bound by a factor of at least 4 on one logit set or more (the rule of
    tests/test_clip_stages_host.py).  ``CAUGHT_BY`` below is asserted, not only documented: per mutant, the logit sets on which
    it is 4 x over the bound of the fp16 rows (what the plans' consumers read) on geometry 3x20x13, stride 16, nc 8.

    mutant               uniform   dominant  two_equal ties      offset    spread120 mixed     | uniform, fp32 bound (boxes32)
    bins_interleaved     158       3.1e4     7.8e3     3.2e3     3.7e3     2.6e4     2.6e4     | 799
    swap_bins            41        5.2e3     2.6e3     1.3e3     950       1.1e4     3.1e3     | 205
    no_max               -         -         -         -         inf       -         inf       | -
    anchor_no_half       2.2e3     5.2e3     5.2e3     4.7e3     4.7e3     5.2e3     5.2e3     | 4.7e3
    mod_h                8.3e4     1.9e5     1.9e5     1.7e5     1.5e5     2.0e5     1.3e5     | 1.8e5
    swap_d0_d2           812       9.4e4     1.1e5     2.7e4     3.6e4     1.2e5     6.1e4     | 3.3e3
    swap_wh_rows         147       2.3e5     4.4e4     1.6e3     2.0e3     2.2e5     1.7e5     | 5.6e3
    stride_centre_only   3.6e3     3.8e3     3.5e3     3.7e3     3.7e3     3.6e3     3.8e3     | 1.4e5
    sigmoid_neg          3.4e7     (the class logits are the same in every set)                | 8.5e37
    cls_xor1             3.4e7                                                                 | 8.5e37
    batch0               3.4e7                                                                 | 8.5e37
    (observed / bound; "-": inside the bound, the mutant is invisible there)

    Under these bounds -- 10 to 1000 times tighter than the 0.03 px the whole-plan tests allow -- the near-uniform logits of the seeded
    plans see every mutant but one, by the smallest margins of all sets (41 x for two exchanged bins, where a peaked set gives 5000 x).
    The missing max subtraction changes nothing on them, nor on any set whose logits stay below 88: only the common offset of
    +-1000 exposes it (inf / inf and 0 / 0).  A spread of 120 around zero does not: e**60 is an fp32 number."""
import functools

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd.yolov8 import build_detector_net
from tests import head_refs as R

FACTOR = 4.0
MUT_GEOMETRY, MUT_NC = R.GEOMETRIES[0], 8
ALL = frozenset(R.BOX_SETS)
# mutant -> (sets that catch it on the fp16 rows, caught on the uniform set under the fp32-only bound)
CAUGHT_BY = {
    "bins_interleaved": (ALL, True),
    "swap_bins": (ALL, True),
    "no_max": (frozenset({"offset", "mixed"}), False),
    "anchor_no_half": (ALL, True),
    "mod_h": (ALL, True),
    "swap_d0_d2": (ALL, True),
    "swap_wh_rows": (ALL, True),
    "stride_centre_only": (ALL, True),
    "sigmoid_neg": (ALL, True),
    "cls_xor1": (ALL, True),
    "batch0": (ALL, True),
}


@functools.lru_cache(maxsize=None)
def _case(name, geometry, nc, kind):
    return R.case(name, geometry, nc, kind, R.GEOMETRY_STRIDE[geometry])


def test_head_ref_is_the_module_in_float64():
    net = build_detector_net("n", seed=0).double()
    x = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    with torch.no_grad():
        want = net(x).numpy()
        box, cls = (t.numpy() for t in net(x, raw=True))
    assert want.dtype == np.float64 and box.dtype == np.float64
    a0 = 0
    for stride in (8, 16, 32):
        h, w = 64 // stride, 96 // stride
        lv = slice(a0, a0 + h * w)
        got = R.head_ref(box[:, :, lv].transpose(0, 2, 1).reshape(2, h, w, 64), cls[:, :, lv].transpose(0, 2, 1).reshape(2, h, w, -1),
                         stride)
        assert got.shape == want[:, :, lv].shape
        rel = np.abs(got - want[:, :, lv]) / np.abs(want[:, :, lv])
        print(f"stride {stride}: max relative difference {rel.max():.3e}")
        assert rel.max() < 1e-12
        a0 += h * w
    assert a0 == want.shape[2]


def test_logit_sets_are_what_they_claim():
    B, h, w = MUT_GEOMETRY
    for kind, dtype in (("f16", np.float16), ("f32", np.float32)):
        d = {}
        for name in R.BOX_SETS:
            box = R.box_logits(name, B, h, w, dtype)
            assert box.dtype == dtype and np.isfinite(box).all()
            x, p, d[name] = R._softmax(box)
        v = R.box_logits("uniform", B, h, w, dtype).astype(np.float64).reshape(-1, 16)
        assert (v.max(1) - v.min(1)).max() <= 0.2 and np.abs(d["uniform"] - 7.5).max() < 0.5
        dom = d["dominant"]
        for s in range(4):                                               # every bin dominates on every side
            assert set(np.unique(np.round(dom[..., s]).astype(int))) == set(range(16)) and np.abs(dom - np.round(dom)).max() < 0.01
        assert set(np.unique(d["two_equal"].round(9))) == {t + 0.5 for t in range(15)}
        assert set(np.unique(d["spread120"].round(9))) == set(float(t) for t in range(16))
        ties = R.box_logits("ties", B, h, w, dtype).astype(np.float64).reshape(-1, 16)
        assert set(np.unique((ties == ties.max(1, keepdims=True)).sum(1))) == set(range(2, 17))
        off = R.box_logits("offset", B, h, w, dtype).astype(np.float64)
        assert off.min() == -1000 and off.max() == 1004 and np.all(off == np.round(off))
        # the four sides of an anchor differ
        assert np.mean(np.ptp(d["mixed"], axis=-1) > 0.25) > 0.9
        cls = R.cls_logits(B, h, w, 8, dtype).astype(np.float64)
        for s in (17.0, 88.0, 100.0, 65504.0):
            assert (cls == s).any() and (cls == -s).any()
        assert (cls == 2.0 ** -24).any() and np.any((cls == 0) & np.signbit(cls))
        assert set(np.arange(-320, 321) / 16.0) <= set(np.unique(cls))


@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=R.geometry_id)
def test_faithful_restatement_is_inside_every_bound(geometry):
    bad = []
    for nc in (8, 3):
        for name in R.BOX_SETS:
            for fast, kind in ((True, "f16"), (False, "f32")):
                if kind == "f16" and nc % 8:
                    continue
                box, cls, ref, tol = _case(name, geometry, nc, kind)
                got = R.head_f32_cpu(box, cls, R.GEOMETRY_STRIDE[geometry], fast_exp=fast)
                assert got.dtype == np.float32
                what = f"{R.geometry_id(geometry)} nc {nc} {name}"
                R.check_rows(f"cpu_restatement_{kind}", what + " fp32", got, ref, tol, bad)
                if kind == "f16":
                    R.check_rows("cpu_restatement_f16", what + " stored as fp16", got.astype(np.float16), ref, R.fp16_store_tol(ref, tol), bad)
    assert not bad, bad


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_leaves_the_bound(mut):
    stride = R.GEOMETRY_STRIDE[MUT_GEOMETRY]
    caught16, caught32 = set(), set()
    for name in R.BOX_SETS:
        box, cls, ref, tol = _case(name, MUT_GEOMETRY, MUT_NC, "f16")
        got = R.head_f32_cpu(box, cls, stride, fast_exp=True, mut=mut)
        with np.errstate(over="ignore"):
            r16 = R.ratio(got.astype(np.float16), ref, R.fp16_store_tol(ref, tol))
        r32 = R.ratio(got, ref, tol)
        print(f"{mut} {name}: fp16 rows {r16:.3g} x bound, fp32 {r32:.3g} x bound")
        if r16 >= FACTOR:
            caught16.add(name)
        if r32 >= FACTOR:
            caught32.add(name)
    want16, uniform32 = CAUGHT_BY[mut]
    assert caught16, "no logit set sees this mutant"
    assert caught16 == want16, (sorted(caught16), sorted(want16))
    assert ("uniform" in caught32) == uniform32
    assert caught32 >= caught16


def test_mutants_of_the_fp32_head_order_leave_the_bound_too():
    """The same mutants in k_head_f32's operation order (``fast_exp=False``) against the fp32 head's bound: each is caught on the mixed
    set (the missing max subtraction included)."""
    stride = R.GEOMETRY_STRIDE[MUT_GEOMETRY]
    box, cls, ref, tol = _case("mixed", MUT_GEOMETRY, MUT_NC, "f32")
    for mut in R.MUTANTS:
        r = R.ratio(R.head_f32_cpu(box, cls, stride, fast_exp=False, mut=mut), ref, tol)
        print(f"{mut}: {r:.3g} x bound")
        assert r >= FACTOR, mut
