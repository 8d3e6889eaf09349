"""The slice layouts the fused plans hand the fp16 convolution kernels, shared by tests/test_gpu_conv_slices.py (every row of the
variant table on them, on the GPU) and tests/test_conv_slices_v5_host.py / tests/test_conv_slices_11_host.py (CPU: the bound of
``helpers.assert_conv_close`` rejects planted slice errors on them).

``Layout`` says where a step's input, output and residual lie: (row stride, channel offset) in halves.  Every generator restates
one member of ``Builder`` (csrc/rva_plan.hip) and returns the layouts of the convolution steps it pushes, by role: ``c3_layouts``
``Builder::c3`` (YOLOv5's C3, YOLO11's C3k), ``c3k2_layouts`` ``Builder::c2f`` with the ``block`` lambda of ``Builder::build_11``,
``c2psa_layouts`` ``Builder::c2psa``, ``cls_branch_layouts`` the class branch of ``Builder::build_11``; ``b1_layout`` /
``h10_layout`` are the two steps of ``Builder::build_v5`` that the YOLOv8 builder has no like of.  ``make_case`` /
``conv_slice_f32_cpu`` are the host side: seeded operands in plan-shaped flat buffers and the kernel restated in float32 through
the slice arithmetic, with a ``mut=`` hook that plants one error (as ``yolov5_refs.stem6_f32_cpu`` does)."""
from typing import NamedTuple, Optional, Tuple


class Layout(NamedTuple):
    name: str
    cin: int                                   # real input channels (the reference reads these)
    cin_decl: int                              # what the step declares: Cin rounded up to 32 (Builder::conv), zero weight columns
    cout: int
    k: int
    stride: int
    act: int
    inp: Tuple[int, int]                       # (row stride, channel offset) of the input slice
    out: Tuple[int, int]                       # ... of the output slice
    res: Optional[Tuple[int, int]] = None      # ... of the residual slice
    res_own: bool = False                      # False: the residual lives in the OUTPUT allocation (Builder::c2f, a C3 with one
                                               # bottleneck); True: in a buffer of its own (Builder::c3 with two or more)
    live: Optional[Tuple[int, int]] = None     # (cin, cout) of the checkpoint's convolution where Builder::padded zero-extends it
                                               # to (cin, cout): the weight rows, columns and biases past `live` are zero


def _decl(c):
    return (c + 31) // 32 * 32                 # Builder::conv: `s.Cin = (s.Cin + 31) / 32 * 32`


def c3_layouts(c1, c2, n, shortcut, tag, k1=1, src=None, dst=None, family="v5"):
    """``Builder::c3(n, shortcut, src, dst, l, what, k1)``: the convolution steps it pushes, by role.  ``src`` / ``dst`` are
    (row stride, offset) of its input and output views, one contiguous buffer each where not given (YOLOv5); YOLO11's C3k
    (``k1 = 3``) gets slices of the outer C2f row.  ``cat`` is the block's 3c-channel buffer; every bottleneck but the last
    writes a c-channel buffer of its own."""
    src, dst = src or (c1, 0), dst or (c2, 0)
    c = c2 // 2                                                                               # `c = c2 / 2`
    cat = 3 * c                                                                               # `View cat = buf(l, 3 * c)`
    what = f"{family} {tag} c{c}"
    out = {
        # `conv_in(cv, 2, src, cat.sub(0, 2 * c), l)`: cv1 | cv2 as one convolution into the front of the row
        "cv1|cv2": Layout(f"{what} cv1|cv2", c1, _decl(c1), 2 * c, 1, 1, 1, src, (cat, 0)),
    }
    x, x_in_cat = (cat, 0), True                                                              # `View x = cat.sub(0, c)`
    for i in range(n):
        last = i == n - 1
        y = (cat, 2 * c) if last else (c, 0)                                                  # `y = i == n - 1 ? cat.sub(2 * c, c) : buf(l, c)`
        # Builder::bottleneck, `conv1(b1, x, tmp, l, 1)`: k1 x k1 from x into the contiguous tmp
        out[f"m{i}.cv1"] = Layout(f"{what} m{i}.cv1 of {n}", c, _decl(c), c, k1, 1, 1, x, (c, 0))
        # Builder::bottleneck, `conv1(b2, tmp, y, l, 1, shortcut ? &x : nullptr)`: x and y share an allocation only where both are
        # slices of cat (n = 1)
        out[f"m{i}.cv2"] = Layout(f"{what} m{i}.cv2 of {n}" + ("" if shortcut else " no shortcut"), c, _decl(c), c, 3, 1, 1, (c, 0), y,
                                  x if shortcut else None, shortcut and not (x_in_cat and last))
        x, x_in_cat = y, last                                                                 # `x = y`
    # `conv1(..., cat.sub(c, 2 * c), dst, l, 1)`: [cv2 out | m out] from the middle of the row
    out["cv3"] = Layout(f"{what} cv3", 2 * c, _decl(2 * c), c2, 1, 1, 1, (cat, c), dst)
    return out


def b1_layout(c1, c2, tag):
    """Builder::stem, `conv1(b1, x0, *x1, 1, 1)`: contiguous stem output in, Cin declared up to 32."""
    return Layout(f"v5 {tag} b1 {c1}->{c2}", c1, _decl(c1), c2, 3, 2, 1, (c1, 0), (c2, 0))


def h10_layout(c4, c5, tag):
    """Builder::build_v5, `conv1(take(c5, c4, 1, 1, "h10"), p5, t10, 5, 1)` with t10 = cat23.sub(c4, c4): the back half of a concat row."""
    return Layout(f"v5 {tag} h10 {c5}->{c4}", c5, _decl(c5), c4, 1, 1, 1, (c5, 0), (2 * c4, c4))


# The C3 blocks the layouts below are taken from.  YOLOv5n: widths 16 32 64 128 256, depths 1 2 3 1; YOLOv5m: 48 96 192 384 768,
# depths 2 4 6 2.  Two blocks are not in a stock model: the widths of n's / m's b2 with the other's depth, so that c = 16 meets a
# residual in another allocation and c = 48 one in the same.
N_B2 = c3_layouts(32, 32, 1, True, "n b2")
N_B4 = c3_layouts(64, 64, 2, True, "n b4")
N_B6 = c3_layouts(128, 128, 3, True, "n b6")
N_H17 = c3_layouts(128, 64, 1, False, "n h17")         # its cv1|cv2 is an upsample + concat step: only the bottleneck is taken
N_H20 = c3_layouts(128, 128, 1, False, "n h20")        # src = the whole cat20
M_B2 = c3_layouts(96, 96, 2, True, "m b2")
C16_N2 = c3_layouts(32, 32, 2, True, "n b2 x2")
C48_N1 = c3_layouts(96, 96, 1, True, "m b2 x1")

V5_STRIDE1_LAYOUTS = [
    # 1: sibling cv1|cv2 into the front 2c of a 3c row
    N_B2["cv1|cv2"], M_B2["cv1|cv2"], N_H20["cv1|cv2"],
    # 2: bottleneck cv1 on the front slice of the 3c row: c = 16 / 48 declared 32 / 64 read into the cv2 half
    N_B2["m0.cv1"], M_B2["m0.cv1"], N_B6["m0.cv1"],
    # 3: first bottleneck of two or more: shortcut from cat.sub(0, c) (row stride 3c), output a buffer of its own (row stride c)
    C16_N2["m0.cv2"], M_B2["m0.cv2"], N_B6["m0.cv2"],
    # 4: a middle bottleneck: shortcut from the previous bottleneck's buffer
    N_B6["m1.cv2"],
    # 5: the last of two or more: writes cat.sub(2c, c), shortcut in another allocation
    C16_N2["m1.cv2"], N_B6["m2.cv2"],
    # 6: the only bottleneck: shortcut cat.sub(0, c) and output cat.sub(2c, c) in one allocation
    N_B2["m0.cv2"], C48_N1["m0.cv2"],
    # 7: neck C3, no shortcut
    N_H17["m0.cv2"],
    # 8: cv3 from the middle of the row
    N_B2["cv3"], M_B2["cv3"], N_B6["cv3"],
    # 9: h10 of YOLOv5n into the back half of cat23
    h10_layout(128, 256, "n"),
]
V5_STRIDE2_LAYOUTS = [b1_layout(16, 32, "n"), b1_layout(48, 96, "m")]          # 10, 11


# ---------------------------------------------------------------------------------------------------------------- YOLO11
def c3k2_layouts(c1, c2, n, c3k, shortcut, quarter, tag):
    """``Builder::c2f(c, n, src, dst, l, what, inner)`` as the ``block`` lambda of ``Builder::build_11`` calls it, with ``src`` and
    ``dst`` one contiguous view each: the convolution steps it pushes, by role.  ``cat`` is the block's (2 + n) c row.  The inner
    blocks are ``Builder::bottleneck(x, y, c / 2, shortcut, ...)`` -- its intermediate a contiguous c / 2 buffer -- or, with
    ``c3k``, ``Builder::c3(2, shortcut, x, y, l, what, 3)``, whose steps are keyed ``m<i>.<role>``."""
    c = c2 // 4 if quarter else c2 // 2                                 # build_11: `c = i < 2 ? dst.ch / 4 : dst.ch / 2`
    cat = (2 + n) * c                                                   # c2f: `View cat = buf(l, (2 + n) * c)`
    what = f"11 {tag} c{c}"
    # c2f: `conv_in(&cv1, 1, src, cat.sub(0, 2 * c), l)`
    out = {"cv1": Layout(f"{what} cv1", c1, _decl(c1), 2 * c, 1, 1, 1, (c1, 0), (cat, 0))}
    for i in range(n):
        x, y = (cat, (1 + i) * c), (cat, (2 + i) * c)                   # c2f: `inner(cat.sub((1 + i) * c, c), cat.sub((2 + i) * c, c))`
        if c3k:
            for role, lay in c3_layouts(c, c, 2, shortcut, f"{tag} m{i}", k1=3, src=x, dst=y, family="11").items():
                out[f"m{i}.{role}"] = lay
            continue
        h = c // 2
        # bottleneck: `conv1(b1, x, tmp, l, 1)` with tmp = buf(l, cmid)
        out[f"m{i}.cv1"] = Layout(f"{what} m{i}.cv1 {c}->{h}", c, _decl(c), h, 3, 1, 1, x, (h, 0))
        # bottleneck: `conv1(b2, tmp, y, l, 1, shortcut ? &x : nullptr)`: x and y are neighbouring slices of cat
        out[f"m{i}.cv2"] = Layout(f"{what} m{i}.cv2 {h}->{c}" + ("" if shortcut else " no shortcut"), h, _decl(h), c, 3, 1, 1, (h, 0), y,
                                  x if shortcut else None, False)
    # c2f: `conv1(cv2, cat, dst, l, 1)`
    out["cv2"] = Layout(f"{what} cv2", cat, _decl(cat), c2, 1, 1, 1, (cat, 0), (c2, 0))
    return out


def c2psa_layouts(c1, n, tag):
    """``Builder::c2psa(n, heads, src, dst)``: its convolution steps, by role (attention and the depthwise positional encoding
    are not in the variant table).  ``cat`` is cv2's 2c input row; every other buffer is contiguous."""
    c = c1 // 2                                                         # `c = c1 / 2`
    what = f"11 {tag} psa c{c}"
    out = {
        # `conv1(&qa, src, cat.sub(0, c), l, 1)` and `conv1(&qb, src, x, l, 1)`: cv1 as two launches
        "cv1.a": Layout(f"{what} cv1.a", c1, _decl(c1), c, 1, 1, 1, (c1, 0), (2 * c, 0)),
        "cv1.b": Layout(f"{what} cv1.b", c1, _decl(c1), c, 1, 1, 1, (c1, 0), (c, 0)),
    }
    for i in range(n):
        y = (2 * c, c) if i == n - 1 else (c, 0)                        # `y = i == n - 1 ? cat.sub(c, c) : buf(l, c)`
        m = f"{what} m{i} of {n}"
        # `conv1(qkv, x, q, l, 0)`
        out[f"m{i}.qkv"] = Layout(f"{m} qkv", c, _decl(c), 2 * c, 1, 1, 0, (c, 0), (2 * c, 0))
        # `conv1(proj, xo, x1, l, 0, &x)`: x is cv1.b's buffer or the previous block's y, never a slice of cat
        out[f"m{i}.proj"] = Layout(f"{m} proj", c, _decl(c), c, 1, 1, 0, (c, 0), (c, 0), (c, 0), True)
        # `conv1(f0, x1, f, l, 1)`
        out[f"m{i}.ffn.0"] = Layout(f"{m} ffn.0", c, _decl(c), 2 * c, 1, 1, 1, (c, 0), (2 * c, 0))
        # `conv1(f1, f, y, l, 0, &x1)`
        out[f"m{i}.ffn.1"] = Layout(f"{m} ffn.1", 2 * c, _decl(2 * c), c, 1, 1, 0, (2 * c, 0), y, (c, 0), True)
    # `conv1(cv2, cat, dst, l, 1)`
    out["cv2"] = Layout(f"{what} cv2", 2 * c, _decl(2 * c), c1, 1, 1, 1, (2 * c, 0), (c1, 0))
    return out


def cls_branch_layouts(ch, nc, tag, c3=None):
    """The two pointwise steps of the class branch of ``Builder::build_11`` on a level that is ``ch`` channels wide (``c3``: the
    model's stride-8 width, ``ch`` itself where not given).  ``Builder::head_open`` rounds the branch's interior width
    ``cr = max(c3, min(nc, 100))`` up to ``cc``, a multiple of 8; ``Builder::padded`` zero-extends the weights (``live``)."""
    cr = max(c3 or ch, min(nc, 100))                                    # head_open: `hd.cc_real = std::max(g.c[3], ncm)`
    cc = (cr + 7) // 8 * 8                                              # head_open: `hd.cc = (hd.cc_real + cal - 1) / cal * cal`
    what = f"11 {tag} cls nc{nc}"
    return {
        # `conv1(cls[l][1], d1, k1, L, 1)` with cls[l][1] = padded(cls[l][1], ch, cc)
        "0.1": Layout(f"{what} 0.1 {ch}->{cc}", ch, _decl(ch), cc, 1, 1, 1, (ch, 0), (cc, 0), live=(ch, cr)),
        # `conv1(cls[l][3], d2, k2, L, 1)` with cls[l][3] = padded(cls[l][3], cc, cc)
        "1.1": Layout(f"{what} 1.1 {cc}->{cc}", cc, _decl(cc), cc, 1, 1, 1, (cc, 0), (cc, 0), live=(cr, cr)),
    }


# The blocks the layouts below are taken from, named after the module number.  YOLO11n: widths 16 32 64 128 256, C3k in `6`, `8`
# and `22`; YOLO11s: 32 64 128 256 512; YOLO11m: 64 128 256 512 512, C3k everywhere.  Every C3k2 has one inner block.
N11_2 = c3k2_layouts(32, 64, 1, False, True, True, "n 2")              # c 16, row 48, bottleneck 16 -> 8 -> 16
N11_4 = c3k2_layouts(64, 128, 1, False, True, True, "n 4")             # c 32, row 96, bottleneck 32 -> 16 -> 32
S11_4 = c3k2_layouts(128, 256, 1, False, True, True, "s 4")            # c 64, row 192, bottleneck 64 -> 32 -> 64
N11_6 = c3k2_layouts(128, 128, 1, True, True, False, "n 6")            # c 64, row 192, nested c' 32
N11_8 = c3k2_layouts(256, 256, 1, True, True, False, "n 8")            # c 128, row 384, nested c' 64
N11_16 = c3k2_layouts(256, 64, 1, False, False, False, "n 16")         # neck: c 32, no shortcut; its cv1 is an upsample + concat step
N11_22 = c3k2_layouts(384, 256, 1, True, False, False, "n 22")         # neck: nested c' 64, no shortcut
M11_4 = c3k2_layouts(256, 512, 1, True, True, True, "m 4")             # c 128, row 384, nested c' 64: the widest nested block
N11_PSA = c2psa_layouts(256, 1, "n")                                   # c 128
L11_PSA = c2psa_layouts(256, 2, "n x2")                                # two PSA blocks (scales l, x) at n's width
N11_CLS = cls_branch_layouts(64, 80, "n")                              # cc = 80
N11_CLS85 = cls_branch_layouts(64, 85, "n")                            # cr = 85, cc = 88

V11_STRIDE1_LAYOUTS = [
    # 1: cv1 into the front 2c of a (2 + n) c row
    N11_2["cv1"], N11_4["cv1"],
    # 2: bottleneck first conv c -> c / 2, input a middle slice of the row
    N11_2["m0.cv1"], N11_4["m0.cv1"], S11_4["m0.cv1"],
    # 3: bottleneck second conv c / 2 -> c: contiguous c / 2 input (8 and 16 declared 32), output and shortcut neighbouring slices
    N11_2["m0.cv2"], N11_4["m0.cv2"], S11_4["m0.cv2"], N11_16["m0.cv2"],
    # 4: closing cv2 over the whole row, 48 declared 64
    N11_2["cv2"],
    # 5: nested C3k: sibling cv1|cv2 from a slice of the outer row
    N11_6["m0.cv1|cv2"], M11_4["m0.cv1|cv2"],
    # 6: nested C3k: 3x3 -> 3x3 bottlenecks.  m0 reads the front of the 3c' row and writes a buffer of its own, m1 writes back into
    # the row; both shortcuts are in another allocation
    N11_6["m0.m0.cv1"], N11_6["m0.m0.cv2"], N11_6["m0.m1.cv2"], N11_8["m0.m0.cv1"], N11_8["m0.m0.cv2"], N11_8["m0.m1.cv2"],
    N11_22["m0.m1.cv2"],
    # 7: nested C3k: cv3 from the middle of the inner row into a slice of the outer row
    N11_6["m0.cv3"], M11_4["m0.cv3"],
    # 8: C2PSA cv1 as two launches
    N11_PSA["cv1.a"], N11_PSA["cv1.b"],
    # 9: qkv, no activation
    N11_PSA["m0.qkv"],
    # 10: proj, no activation, residual in a buffer of its own with ldr = ldo
    N11_PSA["m0.proj"],
    # 11: ffn.1, no activation, residual of row stride c: of the last block into the back half of the 2c row (ldr != ldo), of an
    # earlier block into a buffer of its own
    N11_PSA["m0.ffn.1"], L11_PSA["m0.ffn.1"],
    # 12: class-branch pointwise, zero-extended to cc
    N11_CLS["0.1"], N11_CLS["1.1"], N11_CLS85["0.1"], N11_CLS85["1.1"],
]
# The stride-2 3x3 steps of build_11 (Builder::stem, Builder::backbone, Builder::bottom_up) read a contiguous buffer whose Cin is
# declared up to 32 (16 -> 32, as b1 of YOLOv5n above), a contiguous buffer or the back half of a neck concat row (as b5), and write
# a contiguous buffer or the front of a concat row (as h16): every kind is in STRIDE2_LAYOUTS of tests/test_gpu_conv_slices.py
# already, so there is none to add.
V11_STRIDE2_LAYOUTS = []


# ---------------------------------------------------------------------------------------------------------------- host side
SLACK = 32                                    # halves behind every plan buffer (Builder::buf: 64 bytes)
MUTANTS = ("ldr_is_ldo", "drop_last_8", "input_offset_ignored", "pad_columns_live", "silu_despite_act0")


def out_hw(lay, H, W):
    k, s = lay.k, lay.stride
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def zero_extend(lay, w, b):
    """``w`` [cout, cin, k, k] and ``b`` [cout] as ``Builder::padded`` leaves them: zero past ``lay.live``.  In place."""
    if lay.live is not None:
        cin, cout = lay.live
        w[:, cin:] = 0
        w[cout:] = 0
        b[cout:] = 0
    return w, b


def make_case(lay, shape, seed=11):
    """Seeded operands for ``lay`` at ``shape`` = (B, H, W): the input and residual as flat fp16 plan buffers (rows of the full
    row stride, every channel random, ``SLACK`` zero halves behind), fp16 weights [cout, cin, k, k] of the REAL channels (zero past
    ``lay.live``), an fp32 bias, and the float64 convolution of the real channels of the declared slices (``want``) with the
    residual rows (``res``)."""
    import torch
    import torch.nn.functional as F
    B, H, W = shape
    Ho, Wo = out_hw(lay, H, W)
    Mi, Mo = B * H * W, B * Ho * Wo
    (ldi, offi) = lay.inp
    g = torch.Generator().manual_seed(seed)
    x_rows = (torch.randn((Mi, ldi), generator=g) * 0.5).half()
    w = (torch.randn((lay.cout, lay.cin, lay.k, lay.k), generator=g) / (lay.cin * lay.k * lay.k) ** 0.5).half()
    b = torch.randn((lay.cout,), generator=g) * 0.1
    w, b = zero_extend(lay, w, b)
    xs = x_rows[:, offi:offi + lay.cin].reshape(B, H, W, lay.cin).double().permute(0, 3, 1, 2)
    y = F.conv2d(xs, w.double(), b.double(), stride=lay.stride, padding=lay.k // 2)
    if lay.act:
        y = y * torch.sigmoid(y)
    want = y.permute(0, 2, 3, 1).reshape(Mo, lay.cout)
    res = res_flat = None
    if lay.res is not None:
        ldr, offr = lay.res
        res_rows = (torch.randn((Mo, ldr), generator=g) * 0.5).half()
        res = res_rows[:, offr:offr + lay.cout].contiguous()
        want = want + res.double()
        res_flat = torch.cat((res_rows.reshape(-1), torch.zeros(SLACK, dtype=torch.float16)))
    x_flat = torch.cat((x_rows.reshape(-1), torch.zeros(SLACK, dtype=torch.float16)))
    return dict(x_flat=x_flat, w=w, b=b, res_flat=res_flat, res=res, want=want)


def conv_slice_f32_cpu(lay, shape, case, mut=None):
    """The kernel on the CPU: every pixel reads ``cin_decl`` halves from ``pixel * ldi + offset`` of the flat input (past a narrower
    slice into whatever follows, as the step does), the weights are packed with zero columns up to ``cin_decl`` (Builder::pack), the
    sum is fp32, bias and SiLU in fp32, ONE rounding to fp16; the residual is read from ``pixel * ldr + offset``, added in fp32 and
    the sum rounded once more.  Returns [Mo, cout] fp16.  ``mut`` plants one error:
    ``ldr_is_ldo`` the residual read with the output's row stride; ``drop_last_8`` the last 8 real input channels not summed;
    ``input_offset_ignored`` the input read from channel 0 of the row; ``pad_columns_live`` the weight columns cin.. hold the
    weights of the first real columns instead of zeros; ``silu_despite_act0`` SiLU applied where the step says no activation."""
    import torch
    import torch.nn.functional as F
    assert mut in (None,) + MUTANTS
    B, H, W = shape
    Ho, Wo = out_hw(lay, H, W)
    Mi, Mo = B * H * W, B * Ho * Wo
    ldi, offi = lay.inp
    if mut == "input_offset_ignored":
        offi = 0
    idx = torch.arange(Mi).reshape(Mi, 1) * ldi + offi + torch.arange(lay.cin_decl).reshape(1, -1)
    assert int(idx.max()) < case["x_flat"].numel()
    x = case["x_flat"][idx].float().reshape(B, H, W, lay.cin_decl).permute(0, 3, 1, 2)
    wp = torch.zeros((lay.cout, lay.cin_decl, lay.k, lay.k))
    wp[:, :lay.cin] = case["w"].float()
    if mut == "drop_last_8":
        wp[:, lay.cin - 8:lay.cin] = 0.0
    if mut == "pad_columns_live":
        assert lay.cin_decl > lay.cin
        wp[:, lay.cin:] = wp[:, :lay.cin_decl - lay.cin].clone()        # the two ranges overlap where cin < cin_decl / 2
    y = F.conv2d(x, wp, case["b"].float(), stride=lay.stride, padding=lay.k // 2)
    if mut == "silu_despite_act0":
        assert not lay.act
    if lay.act or mut == "silu_despite_act0":
        y = y * torch.sigmoid(y)
    y = y.permute(0, 2, 3, 1).reshape(Mo, lay.cout).half()
    if lay.res is not None:
        ldr, offr = lay.res
        if mut == "ldr_is_ldo":
            ldr = lay.out[0]
        ridx = torch.arange(Mo).reshape(Mo, 1) * ldr + offr + torch.arange(lay.cout).reshape(1, -1)
        if mut == "ldr_is_ldo":                # with ldo > ldr the wrong stride leaves the buffer: whatever is there, here the buffer again
            ridx = ridx % case["res_flat"].numel()
        assert int(ridx.max()) < case["res_flat"].numel()
        y = (y.float() + case["res_flat"][ridx].float()).half()
    return y
