"""The slice layouts the fused plans hand the fp16 convolution kernels, shared by tests/test_gpu_conv_slices.py (every row of the
variant table on them, on the GPU) and tests/test_conv_slices_v5_host.py (CPU: the bound of ``helpers.assert_conv_close`` rejects
planted slice errors on them).

``Layout`` says where a step's input, output and residual lie: (row stride, channel offset) in halves.  ``c3_layouts`` restates
``Builder::c3`` (csrc/rva_plan.hip:316-348) and returns the layouts of the steps it pushes; ``b1_layout`` / ``h10_layout`` are the
two steps of ``build_v5`` that the YOLOv8 builder has no like of.  ``make_case`` / ``conv_slice_f32_cpu`` are the host side: seeded
operands in plan-shaped flat buffers and the kernel restated in float32 through the slice arithmetic, with a ``mut=`` hook that
plants one error (as ``yolov5_refs.stem6_f32_cpu`` does)."""
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


def _decl(c):
    return (c + 31) // 32 * 32                 # rva_plan.hip:253


def c3_layouts(c1, c2, n, shortcut, tag):
    """``Builder::c3(c1, c2, n, shortcut, src, ...)`` with ``src`` one contiguous view: the convolution steps it pushes, by role.
    ``cat`` is the block's 3c-channel buffer; every bottleneck but the last writes a c-channel buffer of its own."""
    c = c2 // 2                                                                               # rva_plan.hip:322
    cat = 3 * c                                                                               # :327
    what = f"v5 {tag} c{c}"
    out = {
        # :330 `conv(cv, 2, *src, cat.sub(0, 2 * c), ...)`: cv1 | cv2 as one convolution into the front of the row
        "cv1|cv2": Layout(f"{what} cv1|cv2", c1, _decl(c1), 2 * c, 1, 1, 1, (c1, 0), (cat, 0)),
    }
    x, x_in_cat = (cat, 0), True                                                              # :331 `x = cat.sub(0, c)`
    for i in range(n):
        last = i == n - 1
        y = (cat, 2 * c) if last else (c, 0)                                                  # :336
        # :338 `conv1(b1, x, tmp, ...)`: 1x1 from x into the contiguous tmp
        out[f"m{i}.cv1"] = Layout(f"{what} m{i}.cv1 of {n}", c, _decl(c), c, 1, 1, 1, x, (c, 0))
        # :338 `conv1(b2, tmp, y, ..., shortcut ? &x : nullptr)`: x and y share an allocation only where both are slices of cat (n = 1)
        out[f"m{i}.cv2"] = Layout(f"{what} m{i}.cv2 of {n}" + ("" if shortcut else " no shortcut"), c, _decl(c), c, 3, 1, 1, (c, 0), y,
                                  x if shortcut else None, shortcut and not (x_in_cat and last))
        x, x_in_cat = y, last                                                                 # :339
    # :347 `conv1(..., cat.sub(c, 2 * c), dst, ...)`: [cv2 out | m out] from the middle of the row
    out["cv3"] = Layout(f"{what} cv3", 2 * c, _decl(2 * c), c2, 1, 1, 1, (cat, c), (c2, 0))
    return out


def b1_layout(c1, c2, tag):
    """rva_plan.hip:377 `conv1(take(c1, c2, 3, 2, "b1"), x0, x1, ...)`: contiguous stem output in, Cin declared up to 32."""
    return Layout(f"v5 {tag} b1 {c1}->{c2}", c1, _decl(c1), c2, 3, 2, 1, (c1, 0), (c2, 0))


def h10_layout(c4, c5, tag):
    """rva_plan.hip:410,413 `conv1(take(c5, c4, 1, 1, "h10"), p5, t10, ...)` with t10 = cat23.sub(c4, c4): the back half of a concat row."""
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


# ---------------------------------------------------------------------------------------------------------------- host side
SLACK = 32                                    # halves behind every plan buffer (Builder::buf: 64 bytes)
MUTANTS = ("ldr_is_ldo", "drop_last_8", "input_offset_ignored", "pad_columns_live")


def out_hw(lay, H, W):
    k, s = lay.k, lay.stride
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def make_case(lay, shape, seed=11):
    """Seeded operands for ``lay`` at ``shape`` = (B, H, W): the input and residual as flat fp16 plan buffers (rows of the full
    row stride, every channel random, ``SLACK`` zero halves behind), fp16 weights [cout, cin, k, k] of the REAL channels, an fp32
    bias, and the float64 convolution of the real channels of the declared slices (``want``) with the residual rows (``res``)."""
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
    weights of the first real columns instead of zeros."""
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
        wp[:, lay.cin:] = wp[:, :lay.cin_decl - lay.cin]
    y = F.conv2d(x, wp, case["b"].float(), stride=lay.stride, padding=lay.k // 2)
    if lay.act:
        y = y * torch.sigmoid(y)
    y = y.permute(0, 2, 3, 1).reshape(Mo, lay.cout).half()
    if lay.res is not None:
        ldr, offr = lay.res
        if mut == "ldr_is_ldo":
            ldr = lay.out[0]
        ridx = torch.arange(Mo).reshape(Mo, 1) * ldr + offr + torch.arange(lay.cout).reshape(1, -1)
        assert int(ridx.max()) < case["res_flat"].numel()
        y = (y.float() + case["res_flat"][ridx].float()).half()
    return y
