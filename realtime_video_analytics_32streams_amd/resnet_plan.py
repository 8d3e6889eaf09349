"""fp32 ResNet-18 plan: a thin caller of ``rva_resnet_plan_*`` (include/rva.h, kernels in ``csrc/rva_resnet.hip``).

The whole network of :class:`classify.ResNet18` -- the 7x7 stem with its max pool, the eight BasicBlocks with their three
shortcut convolutions, the spatial mean, the linear head -- and the top-k of the ResNet head run as librva kernels that read
planar fp32 frames (what K1 writes) through a device table of frame indices.  What stays here:

  * :func:`pack_resnet18`: the module's tensors in the ABI's order and layouts, every BatchNorm folded in float64 and rounded
    once to fp32;
  * :func:`resnet_flops`: the FLOP count per layer (tools/resnet_plan_report.py);
  * :class:`FusedResNet18`: owns one plan (weights and the workspace for ``max_frames`` frames) and its logits buffer.

``hip_engine: plan`` with ``model_type: resnet`` selects it (:class:`classify.HipResNetDetector`, engine ``"resnet-f32"``).

With ``half: true`` and the detector key ``hip_resnet_fp16: true`` (``hip_engine: plan`` or ``native``) the same head runs as the
fp16 MFMA plan ``rva_resnet_f16_plan_*`` (``csrc/rva_resnet_f16.hip``, engine ``"resnet-f16"``): ``pack_resnet18(net, half=True)``
and :class:`FusedResNet18F16`.

Any other ResNet of the torchvision family (:class:`classify.ResNet`: BasicBlock or Bottleneck, 1..64 blocks per stage) runs as the
same engine ``"resnet-f16"`` on ``rva_resnetx_f16_plan_*`` (the same file and kernels): :func:`pack_resnet`,
:func:`resnet_any_flops` and :class:`FusedResNetF16`.  There a block's shortcut convolution runs inside the launch of the block's
closing convolution (one fp32 sum over both), unless ``split_shortcut=True`` asks for the ResNet-18 plan's separate launches.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _native as N
from .clip_plan import _ClipPlan, _fold64, _round_f16, conv_out

ENGINE = "resnet-f32"        # NOT "fused" / "fused-f32": PipelinedTicks reads those names as YOLO plans
ENGINE_F16 = "resnet-f16"    # its fp16 MFMA form (half: true, hip_engine: plan / native, hip_resnet_fp16: true)

WIDTHS = (64, 128, 256, 512)
# launch-order names of the 19 block convolutions' outputs = the taps of rva_resnet_plan_stage
STAGE_CODES = {"pooled": 0, **{f"mid{b}": 1 + b for b in range(8)}, "down2": 9, "down4": 10, "down6": 11,
               **{f"out{b}": 12 + b for b in range(8)}, "feat": 20}


def block_shapes() -> List[Tuple[int, int, int]]:
    """(cin, cout, stride) of the eight BasicBlocks."""
    out, cin = [], 64
    for i, c in enumerate(WIDTHS):
        out += [(cin, c, 1 if i == 0 else 2), (c, c, 1)]
        cin = c
    return out


def resnet_maps(h: int, w: int) -> List[Tuple[int, int]]:
    """(height, width) of the pooled map and of the four stages' maps."""
    m = [(conv_out(conv_out(h, 7, 2, 3), 3, 2, 1), conv_out(conv_out(w, 7, 2, 3), 3, 2, 1))]
    m.append(m[0])
    for _ in range(3):
        m.append((conv_out(m[-1][0], 3, 2, 1), conv_out(m[-1][1], 3, 2, 1)))
    return m


def resnet_flops(h: int, w: int, classes: int = 1000) -> Dict[str, object]:
    """FLOP (multiply + add = 2) of one frame from the shapes alone: ``stem``, ``convs`` (the 19 block convolutions as ``(name,
    flop, rows per frame, K, Cout)`` in launch order), ``head``, ``frame`` (everything) and the activation floats a frame
    leaves in the plan's workspace."""
    hc, wc = conv_out(h, 7, 2, 3), conv_out(w, 7, 2, 3)
    maps = resnet_maps(h, w)
    stem = 2.0 * hc * wc * 64 * 147
    convs, act = [], maps[0][0] * maps[0][1] * 64 + 512
    for b, (cin, c, stride) in enumerate(block_shapes()):
        ho, wo = maps[1 + b // 2]
        px = ho * wo
        convs.append((f"mid{b}", 2.0 * px * c * 9 * cin, px, 9 * cin, c))
        if cin != c:
            convs.append((f"down{b}", 2.0 * px * c * cin, px, cin, c))
        convs.append((f"out{b}", 2.0 * px * c * 9 * c, px, 9 * c, c))
        act += px * c * (3 if cin != c else 2)
    head = 2.0 * 512 * classes
    return {"stem": stem, "convs": convs, "head": head, "frame": stem + sum(c[1] for c in convs) + head,
            "workspace_floats": act, "frame_bytes": 4.0 * 3 * h * w}


def _is_resnet18(net) -> bool:
    nn = torch.nn
    stem, layers, fc = getattr(net, "stem", None), getattr(net, "layers", None), getattr(net, "fc", None)
    if not (isinstance(stem, nn.Sequential) and len(stem) == 4 and isinstance(layers, nn.Sequential) and len(layers) == 8 and
            isinstance(fc, nn.Linear) and fc.in_features == 512):
        return False
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)  # noqa: E731

    def conv_is(c, cin, cout, k, s, p):
        return isinstance(c, nn.Conv2d) and (c.in_channels, c.out_channels) == (cin, cout) and c.kernel_size == (k, k) and \
            c.stride == (s, s) and c.padding == (p, p) and c.dilation == (1, 1) and c.groups == 1

    bn_is = lambda m, c: isinstance(m, nn.BatchNorm2d) and m.num_features == c and m.track_running_stats  # noqa: E731
    pool = stem[3]
    if not (conv_is(stem[0], 3, 64, 7, 2, 3) and bn_is(stem[1], 64) and isinstance(stem[2], nn.ReLU) and
            isinstance(pool, nn.MaxPool2d) and pair(pool.kernel_size) == (3, 3) and pair(pool.stride) == (2, 2) and
            pair(pool.padding) == (1, 1) and pair(pool.dilation) == (1, 1) and not pool.ceil_mode):
        return False
    for blk, (cin, c, s) in zip(layers, block_shapes()):
        if not all(hasattr(blk, a) for a in ("c1", "b1", "c2", "b2", "down")):
            return False
        if not (conv_is(blk.c1, cin, c, 3, s, 1) and bn_is(blk.b1, c) and conv_is(blk.c2, c, c, 3, 1, 1) and bn_is(blk.b2, c)):
            return False
        if cin != c:
            d = blk.down
            if not (isinstance(d, nn.Sequential) and len(d) == 2 and conv_is(d[0], cin, c, 1, 2, 0) and bn_is(d[1], c)):
                return False
        elif blk.down is not None:
            return False
    return True


def pack_resnet18(net, half: bool = False) -> Dict[str, np.ndarray]:
    """The ``rva_resnet_weights`` arrays of a :class:`classify.ResNet18` (``N.ResNetWeights.NAMES`` order), contiguous fp32, each
    convolution with its BatchNorm folded in float64 and rounded once, in the layouts the kernels read:

      * ``stem_w`` ``[64, 3, 7, 7]`` (the module's own layout: the VALU stem keeps a channel's 147 taps in registers);
      * ``c<i>_w`` ``[Cout, k*k, Cin]`` with ``tap = ky*k + kx`` (channels innermost, as the NHWC activations), ``c<i>_b``
        ``[Cout]``; per block conv1, conv2, then its shortcut where it has one (``c6``, ``c11``, ``c16``);
      * ``head_w`` ``[classes, 512]``, ``head_b`` ``[classes]``.

    ``half=True`` (the fp16 plan): the same names, order and layouts, fp16-representable -- ``stem_w`` and every ``c<i>_w`` are
    folded with their BatchNorm in float64, rounded once to fp16 and widened to fp32 (the values ``rva_resnet_f16_plan_create``
    then converts exactly); a value beyond fp16 raises ``ValueError`` naming the array.  The biases and the head stay fp32."""
    if not _is_resnet18(net):
        raise ValueError("pack_resnet18: not the ResNet18 architecture")
    blocks = ([(blk.c1, blk.b1), (blk.c2, blk.b2)] + ([(blk.down[0], blk.down[1])] if blk.down is not None else []) for blk in net.layers)
    return _pack("pack_resnet18", half, (net.stem[0], net.stem[1]), blocks, net.fc)


def _pack(who: str, half: bool, stem, blocks, fc, fuse: int = 0) -> Dict[str, np.ndarray]:
    """What :func:`pack_resnet18` and :func:`pack_resnet` return, from the ``(conv, bn)`` pair of the stem, per block the list of
    its pairs in the ABI's order (the shortcut last) and the head: every pair folded in float64, the weight rounded once to fp16
    (``half``; ``who`` names the refusal) or to fp32 and laid out ``[Cout, k*k, Cin]``, the bias rounded once to fp32.  ``fuse``:
    a block of more than ``fuse`` pairs has a shortcut whose bias is added, in float64, to that of the pair before it."""
    def fold(conv, bn, what):
        wf, bf = _fold64(conv, bn)
        return (_round_f16(wf.numpy(), what, who) if half else wf.float().numpy()), bf

    out = {}
    out["stem_w"], b = fold(*stem, "stem_w")
    out["stem_b"] = b.float().numpy()
    i = 0
    for pairs in blocks:
        first, biases = i, []
        for conv, bn in pairs:
            w, b = fold(conv, bn, f"c{i}_w")
            out[f"c{i}_w"] = w.reshape(w.shape[0], w.shape[1], -1).transpose(0, 2, 1)    # [co,ci,kk] -> [co,kk,ci]
            biases.append(b)
            i += 1
        if fuse and len(pairs) > fuse:
            biases[-2] = biases[-2] + biases[-1]                       # float64; rounded once below
        for k, b in enumerate(biases):
            out[f"c{first + k}_b"] = b.float().numpy()
    out["head_w"] = fc.weight.detach().float().cpu().numpy()
    out["head_b"] = fc.bias.detach().float().cpu().numpy() if fc.bias is not None else np.zeros(fc.out_features, np.float32)
    names = ["stem_w", "stem_b"] + [f"c{j}_{x}" for j in range(i) for x in "wb"] + ["head_w", "head_b"]
    return {n: np.ascontiguousarray(out[n], dtype=np.float32) for n in names}


class _ResNetPlan(_ClipPlan):
    """What the ResNet plans share over :class:`_ClipPlan`: reading ``_info`` and ``__call__``."""

    def _read_info(self) -> None:
        maps, ws, nl = (C.c_int32 * 10)(), C.c_int64(), C.c_int32()
        self.ctx.check(self._fn("info")(self.handle, maps, C.byref(ws), C.byref(nl)), f"{self.ABI}_info")
        self.maps = [(maps[2 * s], maps[2 * s + 1]) for s in range(5)]
        self.workspace_bytes, self.n_launches = ws.value, nl.value

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        """The network's ``forward`` of frames ``[B, 3, H, W]``: a fresh fp32 ``[B, classes]`` tensor.  An fp32 plan takes fp32
        frames; an fp16 plan takes fp16 frames, or fp32 ones that are rounded to fp16 here."""
        b = int(frames.shape[0])
        if tuple(frames.shape[1:]) != (3, self.H, self.W):
            raise ValueError(f"frames must be [B, 3, {self.H}, {self.W}], got {tuple(frames.shape)}")
        if self.RING_DTYPE == torch.float16:
            frames = frames.to(torch.float16)
        return self._run_frames(frames.contiguous(), b)


class FusedResNet18(_ResNetPlan):
    """One ``rva_resnet_plan``: the fp32 network of ``net`` (a :class:`classify.ResNet18`) for frames of ``hw``, up to
    ``max_frames`` frames per call, with the top ``top_k`` in :meth:`post`.  The surface of the clip plans with ``T = 1``
    (``max_clips`` = frames, ``classes``, ``logits``, ``run``, ``post``, ``stage``, ``__call__``).  No host synchronisation and
    no allocation after construction (capturable)."""

    ABI = "rva_resnet_plan"
    HALF = False                              # pack_resnet18(half=...): the precision of the convolution weights

    def __init__(self, net, hw: Tuple[int, int], max_frames: int, top_k: int = 5, ctx: Optional[N.Context] = None,
                 device: Optional[torch.device] = None):
        packed = pack_resnet18(net, half=self.HALF)                 # a wrong architecture is refused before the device is touched
        self._open(hw, 1, max_frames, net.fc.out_features, ctx, device)
        self.top_k = int(top_k)
        self.k = min(self.top_k, self.classes)
        self._create(N.ResNetDesc(self.H, self.W, self.classes, self.top_k, self.max_clips), N.ResNetWeights, packed)
        self._read_info()

    def stage_shape(self, name: str, n: int) -> tuple:
        if name == "feat":
            return (n, 512)
        if name == "pooled":
            return (n, *self.maps[0], 64)
        b = int(name[-1])
        return (n, *self.maps[1 + b // 2], WIDTHS[b // 2])

    def stage(self, name: str, n: int) -> torch.Tensor:
        """A copy of one intermediate tensor of the last :meth:`run` (of at least ``n`` frames, on the current stream), NHWC, as
        ``rva_resnet_plan_stage`` documents (include/rva.h): ``"pooled"``, ``"mid0"`` .. ``"mid7"``, ``"down2"`` / ``"down4"``
        / ``"down6"``, ``"out0"`` .. ``"out7"``, ``"feat"`` ``[n, 512]``.  A read-only tap for tests and tools."""
        n = int(n)
        stages = {k: (code, self.stage_shape(k, n)) for k, code in STAGE_CODES.items()}
        return self._tap(stages, name, n)


class FusedResNet18F16(FusedResNet18):
    """One ``rva_resnet_f16_plan``: the network of :class:`FusedResNet18` for ``half: true`` -- fp16 frames, fp16 convolution
    weights (``net``'s fp32 parameters folded in float64 and rounded once) and fp16 stored activations on the fp16 MFMA, every
    sum in fp32, fp32 ``out7``, ``feat`` and logits.  Same surface: ``run`` takes fp16 frames, ``stage`` returns every stage but
    ``out7`` and ``feat`` as an fp16 tensor."""

    ABI = "rva_resnet_f16_plan"
    HALF = True
    RING_DTYPE = torch.float16
    TAP_DTYPES = {n: torch.float16 for n in STAGE_CODES if n not in ("out7", "feat")}


# ---------------------------------------------------------------------------------------------------------------------
# any ResNet of the torchvision family (classify.ResNet) on rva_resnetx_f16_plan_*
def resnet_blocks(bottleneck: bool, blocks) -> List[Dict[str, int]]:
    """One dict per block over all stages, in order: ``s`` (stage 0..3), ``cin``, ``width``, ``cout``, ``stride``, ``shortcut``
    (whether it has a shortcut convolution: stride != 1 or cin != cout)."""
    out, cin, exp = [], 64, 4 if bottleneck else 1
    for s, n in enumerate(blocks):
        for j in range(int(n)):
            width, stride = WIDTHS[s], 2 if (j == 0 and s > 0) else 1
            cout = width * exp
            out.append({"s": s, "cin": cin, "width": width, "cout": cout, "stride": stride, "shortcut": int(stride != 1 or cin != cout)})
            cin = cout
    return out


def _is_resnet(net) -> bool:
    from .classify import ResNet
    return isinstance(net, ResNet)


def pack_resnet(net, half: bool = True, fused: bool = True) -> Dict[str, np.ndarray]:
    """The ``rva_resnetx_weights`` arrays of a :class:`classify.ResNet`, contiguous fp32, in the ABI's order: ``stem_w`` ``[64, 3,
    7, 7]`` / ``stem_b``; ``c<i>_w`` ``[Cout, k*k, Cin]`` / ``c<i>_b`` block by block -- conv1, conv2[, conv3], then the block's
    shortcut where it has one; ``head_w`` ``[classes, 512 * expansion]`` / ``head_b``.  Every BatchNorm is folded in float64 and
    rounded once: the weights to fp16 with ``half`` (widened to fp32; a value beyond fp16 raises ``ValueError`` naming the array),
    the biases to fp32.  ``fused`` (what a plan without ``split_shortcut`` reads): the bias of a block's closing convolution is
    ``b_close + b_short``, added in float64 and rounded once to fp32; the shortcut keeps its own bias, which that plan does not read."""
    if not _is_resnet(net):
        raise ValueError(f"pack_resnet: not a classify.ResNet ({type(net).__name__}; classify.ResNet18 is packed by pack_resnet18)")
    own = 3 if net.block == "bottleneck" else 2
    blocks = ([(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)] + ([(blk.conv3, blk.bn3)] if own == 3 else []) +
              ([(blk.downsample[0], blk.downsample[1])] if blk.downsample is not None else [])
              for s in range(4) for blk in getattr(net, f"layer{s + 1}"))
    return _pack("pack_resnet", half, (net.conv1, net.bn1), blocks, net.fc, fuse=own if fused else 0)


def resnet_any_flops(bottleneck: bool, blocks, h: int, w: int, classes: int = 1000, split_shortcut: bool = False) -> Dict[str, object]:
    """FLOP (multiply + add = 2) and the bytes the fp16 plan must at least move per frame, from the shapes alone.  ``launches``:
    the block convolutions in launch order as ``(name, flop, bytes, output pixels, K, Cout)`` with ``K`` the length of an output's
    sum (taps x Cin, plus Cin2 where the launch carries the shortcut) and bytes = the input map(s) and weights read once and the
    output written (fp16; the last block's output fp32), plus the residual a split or identity block reads.  ``stem``, ``head``,
    ``frame`` (all FLOP) and ``workspace_bytes`` (what a frame keeps in the plan's workspace)."""
    hc, wc = conv_out(h, 7, 2, 3), conv_out(w, 7, 2, 3)
    maps = resnet_maps(h, w)
    table = resnet_blocks(bottleneck, blocks)
    launches, ws = [], 2 * maps[0][0] * maps[0][1] * 64 + 4 * table[-1]["cout"]
    hin, win = maps[0]
    for b, t in enumerate(table):
        ho, wo = maps[1 + t["s"]]
        px_in, px = hin * win, ho * wo
        cin, width, cout, last = t["cin"], t["width"], t["cout"], b == len(table) - 1
        e_out = 4 if last else 2

        def conv(name, pin, ci, pout, co, k, extra_k=0, extra_bytes=0, e=2):
            K = k * k * ci + extra_k
            launches.append((name, 2.0 * pout * co * K, 2.0 * (pin * ci + K * co) + e * pout * co + extra_bytes, pout, K, co))
            return e * pout * co

        if bottleneck:
            ws += conv(f"b{b}.mid1", px_in, cin, px_in, width, 1)
            ws += conv(f"b{b}.mid2", px_in, width, px, width, 3)
            close_k = 1
        else:
            ws += conv(f"b{b}.mid1", px_in, cin, px, width, 3)
            close_k = 3
        if t["shortcut"] and split_shortcut:
            ws += conv(f"b{b}.down", px_in, cin, px, cout, 1)
            ws += conv(f"b{b}.out", px, width, px, cout, close_k, extra_bytes=2.0 * px * cout, e=e_out)
        elif t["shortcut"]:
            ws += conv(f"b{b}.out", px, width, px, cout, close_k, extra_k=cin, extra_bytes=2.0 * px * cin, e=e_out)
        else:
            ws += conv(f"b{b}.out", px, width, px, cout, close_k, extra_bytes=2.0 * px * cout, e=e_out)
        hin, win = ho, wo
    stem, head = 2.0 * hc * wc * 64 * 147, 2.0 * table[-1]["cout"] * classes
    return {"stem": stem, "launches": launches, "head": head, "frame": stem + sum(c[1] for c in launches) + head,
            "workspace_bytes": ws, "frame_bytes": 2.0 * 3 * h * w}


class FusedResNetF16(_ResNetPlan):
    """One ``rva_resnetx_f16_plan``: the network of ``net`` (a :class:`classify.ResNet` of any depth) for ``half: true`` with the
    numeric contract and the surface of :class:`FusedResNet18F16` (``run`` on fp16 frames, ``post``, ``stage``, ``__call__``,
    ``maps``, ``workspace_bytes``, ``n_launches``, ``classes``, ``logits``).  A block's shortcut convolution runs inside the launch
    of its closing convolution; ``split_shortcut=True`` launches it on its own, as the ResNet-18 plan does.  Stages: ``"pooled"``,
    ``"b<k>.mid1"``, ``"b<k>.mid2"`` (Bottleneck), ``"b<k>.down"`` (split plans, blocks with a shortcut convolution),
    ``"b<k>.out"`` and ``"feat"``, ``k`` counting the blocks over all stages; fp16 but the last block's ``out`` and ``feat``."""

    ABI = "rva_resnetx_f16_plan"
    RING_DTYPE = torch.float16

    def __init__(self, net, hw: Tuple[int, int], max_frames: int, top_k: int = 5, split_shortcut: bool = False,
                 ctx: Optional[N.Context] = None, device: Optional[torch.device] = None):
        self.split_shortcut = bool(split_shortcut)
        packed = pack_resnet(net, half=True, fused=not self.split_shortcut)   # refusals come before the device is touched
        self.bottleneck, self.blocks = net.block == "bottleneck", tuple(net.blocks)
        self.table = resnet_blocks(self.bottleneck, self.blocks)
        self.c_feat = self.table[-1]["cout"]
        self._open(hw, 1, max_frames, net.fc.out_features, ctx, device)
        self.top_k = int(top_k)
        self.k = min(self.top_k, self.classes)
        n_convs = (len(packed) - 4) // 2
        fp = C.POINTER(C.c_float)
        convs = (N.ResNetConv * n_convs)(*[N.ResNetConv(packed[f"c{i}_w"].ctypes.data_as(fp), packed[f"c{i}_b"].ctypes.data_as(fp))
                                           for i in range(n_convs)])
        wt = N.ResNetXWeights(packed["stem_w"].ctypes.data_as(fp), packed["stem_b"].ctypes.data_as(fp), convs,
                              packed["head_w"].ctypes.data_as(fp), packed["head_b"].ctypes.data_as(fp))
        desc = N.ResNetXDesc(self.H, self.W, self.classes, self.top_k, self.max_clips, int(self.bottleneck), (C.c_int32 * 4)(*self.blocks),
                             n_convs, N.RVA_RESX_SPLIT_SHORTCUT if self.split_shortcut else 0)
        h = C.c_void_p()
        with torch.cuda.device(self.dev):
            self.ctx.check(self._fn("create")(self.ctx.handle, C.byref(desc), C.byref(wt), C.byref(h)), f"{self.ABI}_create")
        self.handle = h
        self.logits = torch.empty((self.max_clips, self.classes), dtype=torch.float32, device=self.dev)
        self._read_info()
        self._stages = self._stage_table()
        last = f"b{len(self.table) - 1}.out"
        self.TAP_DTYPES = {n: torch.float16 for n in self._stages if n not in (last, "feat")}

    def _stage_table(self) -> Dict[str, tuple]:
        """name -> (stage code, per-frame shape) of every stage this plan has."""
        out = {"pooled": (N.RVA_RESX_POOLED, (*self.maps[0], 64))}
        hw_in = self.maps[0]
        for b, t in enumerate(self.table):
            hw_out, base = self.maps[1 + t["s"]], N.RVA_RESX_BLOCK0 + 4 * b
            out[f"b{b}.mid1"] = (base, (*(hw_in if self.bottleneck else hw_out), t["width"]))
            if self.bottleneck:
                out[f"b{b}.mid2"] = (base + 1, (*hw_out, t["width"]))
            if t["shortcut"] and self.split_shortcut:
                out[f"b{b}.down"] = (base + 2, (*hw_out, t["cout"]))
            out[f"b{b}.out"] = (base + 3, (*hw_out, t["cout"]))
            hw_in = hw_out
        out["feat"] = (N.RVA_RESX_FEAT, (self.c_feat,))
        return out

    @property
    def stage_names(self) -> Tuple[str, ...]:
        """Every stage of this plan in launch order (``feat`` last)."""
        return tuple(self._stages)

    def stage(self, name: str, n: int) -> torch.Tensor:
        """A copy of one intermediate tensor of the last :meth:`run` (of at least ``n`` frames, on the current stream), NHWC, as
        ``rva_resnetx_f16_plan_stage`` documents (include/rva.h).  A read-only tap for tests and tools."""
        n = int(n)
        return self._tap({k: (code, (n, *shape)) for k, (code, shape) in self._stages.items()}, name, n)
