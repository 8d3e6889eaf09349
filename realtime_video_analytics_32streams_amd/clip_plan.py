"""fp32 CNN-LSTM clip plan: a thin caller of ``rva_cnnlstm_plan_*`` (include/rva.h, kernels in ``csrc/rva_clip.hip``).

The whole clip network of :class:`temporal.CnnLstmNet` -- conv stem with its max pool, conv2 with the spatial mean, the
2-layer LSTM, the linear head -- and the top-5 of the CNN-LSTM head run as librva kernels that read the clip frames straight
from the detector's HBM ring through a device table of frame indices.  What stays here:

  * :func:`pack_cnn_lstm`: the module's tensors in the ABI's order, BatchNorm folded and the two LSTM biases summed in
    float64, each rounded once to fp32;
  * :func:`clip_engine`: which engine a temporal head runs (``hip_engine: plan`` selects this plan for ``cnn_lstm`` with
    ``half: false``);
  * :func:`clip_flops`: the FLOP / byte count of one clip (tools/clip_plan_report.py);
  * :class:`FusedCnnLstm`: owns one plan (weights and the workspace for ``max_clips`` clips) and its logits buffer.

The 3D-CNN head (:class:`temporal.Cnn3dNet`; ``3d_cnn`` and ``slow_fast``) has the same pieces for ``rva_cnn3d_plan_*``
(``csrc/rva_clip3d.hip``, selected by ``hip_engine: native``): :func:`pack_cnn3d`, :func:`clip3d_flops`, :class:`Fused3dCnn`.
With ``half: true`` and the detector key ``hip_clip_fp16: true`` the same head runs as the fp16 MFMA plan ``rva_cnn3d_f16_plan_*``
(``csrc/rva_clip3d.hip``, engine ``"clip3d-f16"``): ``pack_cnn3d(net, half=True)`` and :class:`Fused3dCnnF16`.
The CNN-LSTM head has its fp16 form too: with ``half: true`` and the detector key ``hip_lstm_fp16: true`` it runs as
``rva_cnnlstm_f16_plan_*`` (``csrc/rva_clip_f16.hip``, engine ``"clip-f16"``): ``pack_cnn_lstm(net, half=True)`` and
:class:`FusedCnnLstmF16`.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import ops

LOGGER = logging.getLogger(__name__)

ENGINE = "clip-f32"          # NOT "fused" / "fused-f32": PipelinedTicks reads those names as YOLO plans
ENGINE_F16 = "clip-f16"      # its fp16 MFMA form (half: true, hip_engine: plan / native, hip_lstm_fp16: true)

ENGINE_3D = "clip3d-f32"     # the 3D-CNN plan (3d_cnn / slow_fast, hip_engine: native)
ENGINE_3D_F16 = "clip3d-f16"  # its fp16 MFMA form (half: true, hip_engine: native, hip_clip_fp16: true)


def clip_engine(model_type: str, half: bool, hip_engine: str, has_infer_fn: bool = False, clip_fp16: bool = False,
                lstm_fp16: bool = False) -> str:
    """Engine of a temporal head: ``"infer_fn"`` (a caller's function overrides everything), ``"clip-f32"`` (``cnn_lstm``,
    ``half: false``, ``hip_engine: plan`` or ``native``), ``"clip3d-f32"`` (``3d_cnn`` / ``slow_fast``, ``half: false``,
    ``hip_engine: native``) or ``"torch"``.  ``plan`` is best effort: ``half: true`` on ``cnn_lstm`` raises (the plan is fp32
    only), the other temporal heads keep torch with a warning, so a configuration never changes engines silently.  ``native``
    is strict: the network runs as hand-written HIP at the configured precision or the call raises ``ValueError`` (``half:
    true`` on either plan; ``conv_gru``, for which the reference defines no architecture).  ``clip_fp16`` (the detector key
    ``hip_clip_fp16``) opts ``3d_cnn`` / ``slow_fast`` with ``half: true`` and ``native`` into ``"clip3d-f16"``; it changes nothing
    else.  ``lstm_fp16`` (the detector key ``hip_lstm_fp16``) opts ``cnn_lstm`` with ``half: true`` and ``plan`` or ``native`` into
    ``"clip-f16"``; it changes nothing else either."""
    if has_infer_fn:
        return "infer_fn"
    if hip_engine not in ("plan", "native"):
        return "torch"
    if model_type == "cnn_lstm":
        if half and lstm_fp16:
            return ENGINE_F16
        if half:
            raise ValueError(f"hip_engine: {hip_engine} runs the CNN-LSTM head as an fp32 plan only; set half: false "
                             "(or hip_engine: auto for the PyTorch fp16 network), or hip_lstm_fp16: true for the fp16 plan clip-f16")
        return ENGINE
    if hip_engine == "native":
        if model_type in ("3d_cnn", "slow_fast"):
            if half and clip_fp16:
                return ENGINE_3D_F16
            if half:
                raise ValueError("hip_engine: native runs the 3D-CNN head as an fp32 plan only; set half: false, or "
                                 "hip_clip_fp16: true for the fp16 plan clip3d-f16 (or hip_engine: auto for the PyTorch fp16 "
                                 "network)")
            return ENGINE_3D
        if model_type == "conv_gru":
            raise ValueError("hip_engine: native has no hand-written plan for model_type 'conv_gru': the reference defines no "
                             "architecture for this head (use hip_engine: auto with net=... or infer_fn=...)")
        raise ValueError(f"hip_engine: native has no hand-written plan for model_type {model_type!r}")
    hint = " (hip_engine: native runs it as the fp32 clip3d-f32 plan)" if model_type in ("3d_cnn", "slow_fast") else ""
    LOGGER.warning("hip_engine: plan has no hand-written plan for model_type %r: the network runs through PyTorch-ROCm%s",
                   model_type, hint)
    return "torch"


def conv_out(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def clip_flops(h: int, w: int, frames: int, hidden: int = 512, classes: int = 400, half: bool = False) -> Dict[str, float]:
    """FLOP (multiply + add = 2) and the bytes a clip's network must at least move, from the shapes alone.  ``half``: the byte
    counts of the fp16 plan (fp16 frames, convolution and LSTM weights and ``pooled``; biases and the head fp32)."""
    hc, wc = conv_out(h, 7, 2, 3), conv_out(w, 7, 2, 3)
    hp, wp = conv_out(hc, 3, 2, 1), conv_out(wc, 3, 2, 1)
    conv1 = 2.0 * hc * wc * 64 * 3 * 49
    conv2 = 2.0 * hp * wp * 128 * 64 * 9
    g4 = 4 * hidden
    lstm = 2.0 * frames * (g4 * 128 + g4 * hidden + g4 * 2 * hidden)
    head = 2.0 * hidden * classes
    e = 2.0 if half else 4.0
    weights = e * (64 * 147 + 128 * 576 + g4 * (128 + 3 * hidden)) + 4.0 * (64 + 128 + g4 * 2 + classes * (hidden + 1))
    return {"conv1_per_frame": conv1, "conv2_per_frame": conv2, "frame": conv1 + conv2, "lstm": lstm, "head": head,
            "clip": frames * (conv1 + conv2) + lstm + head, "frame_bytes": e * 3 * h * w, "weight_bytes": weights,
            "lstm_weight_bytes_per_step": e * g4 * 3 * hidden, "pooled_bytes_per_frame": e * hp * wp * 64}


def _fold64(conv, bn) -> Tuple[torch.Tensor, torch.Tensor]:
    """Conv2d / Conv3d with its BatchNorm (eval statistics) folded in, in float64."""
    w = conv.weight.detach().double().cpu()
    b = conv.bias.detach().double().cpu() if conv.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    wf = w * scale.reshape(-1, *([1] * (w.dim() - 1)))
    bf = (b - bn.running_mean.detach().double().cpu()) * scale + bn.bias.detach().double().cpu()
    return wf, bf


def _fold(conv, bn) -> Tuple[np.ndarray, np.ndarray]:
    """:func:`_fold64` rounded once to fp32."""
    wf, bf = _fold64(conv, bn)
    return wf.float().numpy(), bf.float().numpy()


def _round_f16(w, what: str, who: str) -> np.ndarray:
    """``w`` (float64 or fp32) rounded ONCE to fp16, to nearest even, and widened to fp32; a value beyond fp16 raises."""
    with np.errstate(over="ignore"):
        w16 = np.asarray(w).astype(np.float16)
    if not np.isfinite(w16).all():
        raise ValueError(f"{who}: a value of {what} does not stay finite in fp16")
    return w16.astype(np.float32)


def _fold_f16(conv, bn, what: str, who: str = "pack_cnn3d") -> Tuple[np.ndarray, np.ndarray]:
    """:func:`_fold64` with the weight rounded ONCE to fp16 (float64 -> fp16, to nearest even) and widened to fp32; the bias
    rounded once to fp32.  A weight beyond fp16 raises ``ValueError``."""
    wf, bf = _fold64(conv, bn)
    return _round_f16(wf.numpy(), what, who), bf.float().numpy()


def pack_cnn_lstm(net, half: bool = False) -> Dict[str, np.ndarray]:
    """The ``rva_cnnlstm_weights`` arrays of a :class:`temporal.CnnLstmNet` (``N.CnnLstmWeights.NAMES`` order), contiguous fp32.

    ``half=True`` (the fp16 plan): the same names, order and layouts, fp16-representable -- ``conv1_w`` / ``conv2_w`` are folded
    with their BatchNorm in float64 and rounded once to fp16, ``w_ih1`` / ``w_hh1`` / ``w_ih2`` / ``w_hh2`` are rounded once to fp16
    from the module's parameters, each widened to fp32 (the values ``rva_cnnlstm_f16_plan_create`` then converts exactly); a value
    beyond fp16 raises ``ValueError`` naming the array.  The summed LSTM biases, the conv biases and the head stay fp32."""
    st, rnn = net.stem, net.rnn
    if not (isinstance(st[0], torch.nn.Conv2d) and st[0].out_channels == 64 and st[0].kernel_size == (7, 7) and
            isinstance(st[4], torch.nn.Conv2d) and st[4].out_channels == 128 and rnn.num_layers == 2 and rnn.input_size == 128
            and rnn.batch_first and not rnn.bidirectional and rnn.proj_size == 0):
        raise ValueError("pack_cnn_lstm: not the CnnLstmNet architecture")
    p = {n: t.detach().double().cpu() for n, t in rnn.named_parameters()}
    if half:
        c1w, c1b = _fold_f16(st[0], st[1], "conv1_w", "pack_cnn_lstm")
        c2w, c2b = _fold_f16(st[4], st[5], "conv2_w", "pack_cnn_lstm")
    else:
        c1w, c1b = _fold(st[0], st[1])
        c2w, c2b = _fold(st[4], st[5])
    f32 = lambda t: np.ascontiguousarray(t.float().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)  # noqa: E731
    out = {"conv1_w": c1w, "conv1_b": c1b, "conv2_w": c2w, "conv2_b": c2b,
           "w_ih1": p["weight_ih_l0"], "b1": p["bias_ih_l0"] + p["bias_hh_l0"], "w_hh1": p["weight_hh_l0"],
           "w_ih2": p["weight_ih_l1"], "w_hh2": p["weight_hh_l1"], "b2": p["bias_ih_l1"] + p["bias_hh_l1"],
           "head_w": net.head.weight.detach().double().cpu(), "head_b": net.head.bias.detach().double().cpu()}
    if half:
        for k in ("w_ih1", "w_hh1", "w_ih2", "w_hh2"):
            out[k] = _round_f16(out[k].numpy(), k, "pack_cnn_lstm")
    return {n: f32(out[n]) for n in N.CnnLstmWeights.NAMES}


class _ClipPlan:
    """What every clip plan shares, over the ABI entries ``<ABI>_create / _destroy / _run / _run_post / _stage``: the subclass
    sets ``ABI`` and its constructor calls :meth:`_open`, then :meth:`_create` with its descriptor and packed weights."""

    ABI = ""
    RING_DTYPE = torch.float32                # element type of the frame ring ``run`` reads
    TAP_DTYPES: Dict[str, torch.dtype] = {}   # stages whose tap delivers another type than fp32

    def _fn(self, name: str):
        return getattr(self.L, f"{self.ABI}_{name}")

    def _open(self, hw, frames: int, max_clips: int, classes: int, ctx: Optional[N.Context], device: Optional[torch.device]) -> None:
        self.ctx = ctx or ops.context()
        self.dev = device or torch.device("cuda", self.ctx.device)
        self.H, self.W, self.T, self.max_clips, self.classes = int(hw[0]), int(hw[1]), int(frames), int(max_clips), int(classes)
        self.L = N.lib()
        self._iota: Optional[torch.Tensor] = None

    def _create(self, desc, weights_type, packed: Dict[str, np.ndarray]) -> None:
        wt = weights_type(*[packed[n].ctypes.data_as(C.POINTER(C.c_float)) for n in weights_type.NAMES])
        h = C.c_void_p()
        with torch.cuda.device(self.dev):
            self.ctx.check(self._fn("create")(self.ctx.handle, C.byref(desc), C.byref(wt), C.byref(h)), f"{self.ABI}_create")
        self.handle = h
        self.logits = torch.empty((self.max_clips, self.classes), dtype=torch.float32, device=self.dev)

    def __del__(self):  # best effort
        try:
            if getattr(self, "handle", None):
                self._fn("destroy")(self.handle)
                self.handle = None
        except Exception:  # noqa: BLE001
            pass

    def run(self, ring: torch.Tensor, frame_index: torch.Tensor, n_clips: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Logits ``[n_clips, classes]`` of the clips whose frame t of clip b is ``ring.view(-1, 3, H, W)[frame_index[b * T + t]]``,
        launched on the current stream: a view of ``out`` (contiguous fp32 ``[>= n_clips, classes]`` on the device) or of the
        plan's own buffer."""
        if ring.dtype != self.RING_DTYPE or not ring.is_cuda or not ring.is_contiguous() or ring.numel() % (3 * self.H * self.W):
            kind = "fp16" if self.RING_DTYPE == torch.float16 else "fp32"
            raise ValueError(f"ring must be a contiguous {kind} device tensor of [*, 3, {self.H}, {self.W}] frames")
        if frame_index.dtype != torch.int32 or not frame_index.is_cuda or frame_index.numel() < n_clips * self.T:
            raise ValueError("frame_index must be a device int32 tensor of n_clips * T frame indices")
        if not 1 <= n_clips <= self.max_clips:
            raise ValueError(f"n_clips must be in 1..{self.max_clips}, got {n_clips}")
        out = self.logits if out is None else out
        if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or \
                out.shape[1] != self.classes or out.shape[0] < n_clips:
            raise ValueError(f"out must be a contiguous fp32 device tensor of [>= {n_clips}, {self.classes}]")
        self.ctx.check(self._fn("run")(self.handle, C.c_void_p(ring.data_ptr()), C.c_void_p(frame_index.data_ptr()), int(n_clips),
                                       C.c_void_p(out.data_ptr()), ops._stream_ptr()), f"{self.ABI}_run")
        return out[:n_clips]

    def _run_frames(self, frames: torch.Tensor, n_clips: int) -> torch.Tensor:
        """``__call__``: contiguous frames ``[n_clips, T, 3, H, W]`` through the identity index table, a fresh tensor."""
        if self._iota is None:
            self._iota = torch.arange(self.max_clips * self.T, dtype=torch.int32, device=self.dev)
        return self.run(frames, self._iota, n_clips).clone()

    def _tap(self, stages: Dict[str, tuple], name: str, n_clips: int) -> torch.Tensor:
        """``stage()``: the count from a ``dst == NULL`` call, then the one device-to-device copy."""
        fn, what = self._fn("stage"), f"{self.ABI}_stage"
        if name not in stages:
            raise ValueError(f"{what}: unknown stage {name!r} (one of {', '.join(stages)})")
        code, shape = stages[name]
        n = C.c_int64()
        self.ctx.check(fn(self.handle, code, int(n_clips), None, 0, C.byref(n), None), what)
        if n.value != int(np.prod(shape)):
            raise RuntimeError(f"{what}: stage {name} has {n.value} floats, the layout {shape} says {int(np.prod(shape))}")
        out = torch.empty(shape, dtype=self.TAP_DTYPES.get(name, torch.float32), device=self.dev)
        self.ctx.check(fn(self.handle, code, int(n_clips), C.c_void_p(out.data_ptr()), out.numel(), None, ops._stream_ptr()), what)
        return out

    def post(self, logits: torch.Tensor, rows: torch.Tensor, n_rows: int, post: ops.PostBuffers) -> ops.PostBuffers:
        """Top-k result rows into ``post``: ``rows`` = device int32 ``[n_rows, 3]`` of (clip or -1, width, height)."""
        self.ctx.check(self._fn("run_post")(self.handle, C.c_void_p(logits.data_ptr()), C.c_void_p(rows.data_ptr()), int(n_rows),
                                            int(post.max_det), C.c_void_p(post.scores.data_ptr()), C.c_void_p(post.cls.data_ptr()),
                                            C.c_void_p(post.boxes.data_ptr()), C.c_void_p(post.counts.data_ptr()), ops._stream_ptr()),
                       f"{self.ABI}_run_post")
        return post


class FusedCnnLstm(_ClipPlan):
    """One ``rva_cnnlstm_plan``: the fp32 clip network of ``net`` for clips of ``frames`` frames at ``hw``, up to ``max_clips``
    clips per call.  No host synchronisation and no allocation after construction (capturable)."""

    ABI = "rva_cnnlstm_plan"
    HALF = False                              # pack_cnn_lstm(half=...): the precision of the convolution and LSTM weights

    def __init__(self, net, hw: Tuple[int, int], frames: int, max_clips: int, ctx: Optional[N.Context] = None,
                 device: Optional[torch.device] = None):
        packed = pack_cnn_lstm(net, half=self.HALF)                 # a weight beyond fp16 is refused before the device is touched
        self._open(hw, frames, max_clips, net.head.out_features, ctx, device)
        self.hidden = int(net.rnn.hidden_size)
        self._create(N.CnnLstmDesc(self.H, self.W, self.T, self.hidden, self.classes, self.max_clips), N.CnnLstmWeights, packed)
        info = [C.c_int32() for _ in range(4)]
        self.ctx.check(self._fn("info")(self.handle, *[C.byref(v) for v in info]), f"{self.ABI}_info")
        self.pooled_hw = (info[0].value, info[1].value)
        self.conv2_tiles, self.n_launches = info[2].value, info[3].value

    def stage(self, name: str, n_clips: int) -> torch.Tensor:
        """A copy of one intermediate tensor of the last :meth:`run` (of at least ``n_clips`` clips, on the current stream), in
        the layout ``rva_cnnlstm_plan_stage`` documents (include/rva.h): ``"pooled"`` ``[n*T, Hp, Wp, 64]``, ``"partial"``
        ``[n*T, conv2_tiles, 128]``, ``"feat"`` ``[n*T, 128]``, ``"gx"`` ``[n, T, 4*hidden]``, ``"h1"`` / ``"h2"``
        ``[T, n, hidden]``.  A read-only tap for tests and tools."""
        n, T, h = int(n_clips), self.T, self.hidden
        stages = {"pooled": (0, (n * T, *self.pooled_hw, 64)), "partial": (1, (n * T, self.conv2_tiles, 128)),
                  "feat": (2, (n * T, 128)), "gx": (3, (n, T, 4 * h)), "h1": (4, (T, n, h)), "h2": (5, (T, n, h))}
        return self._tap(stages, name, n)

    def __call__(self, clips: torch.Tensor) -> torch.Tensor:
        """``CnnLstmNet.forward`` of contiguous clips ``[B, T, 3, H, W]`` fp32: a fresh ``[B, classes]`` tensor."""
        b = int(clips.shape[0])
        if tuple(clips.shape[1:]) != (self.T, 3, self.H, self.W):
            raise ValueError(f"clips must be [B, {self.T}, 3, {self.H}, {self.W}], got {tuple(clips.shape)}")
        return self._run_frames(clips.contiguous(), b)


class FusedCnnLstmF16(FusedCnnLstm):
    """One ``rva_cnnlstm_f16_plan``: the network of :class:`FusedCnnLstm` for ``half: true`` -- fp16 frames, fp16 convolution and
    LSTM weights (``net``'s fp32 parameters, the convolutions folded in float64, each rounded once) and an fp16 stored ``pooled``,
    conv1 and conv2 on the fp16 MFMA, every sum in fp32, fp32 states and logits.  Same surface: ``run`` takes an fp16 ring,
    ``stage`` returns ``pooled`` as an fp16 tensor."""

    ABI = "rva_cnnlstm_f16_plan"
    HALF = True
    RING_DTYPE = torch.float16
    TAP_DTYPES = {"pooled": torch.float16}

    def __call__(self, clips: torch.Tensor) -> torch.Tensor:
        """``CnnLstmNet.forward`` of clips ``[B, T, 3, H, W]`` of fp16, or of fp32 that is rounded to fp16 here: a fresh fp32
        ``[B, classes]`` tensor."""
        return super().__call__(clips.to(torch.float16))


def clip3d_flops(h: int, w: int, frames: int, classes: int = 400) -> Dict[str, float]:
    """FLOP (multiply + add = 2) and the bytes one 3D-CNN clip must at least move, from the shapes alone.  The pools floor, and
    only the convolution outputs a pool keeps are counted (the plan computes no others)."""
    h1, w1 = h // 2, w // 2
    t2, h2, w2 = frames // 2, h1 // 2, w1 // 2
    conv1 = 2.0 * frames * (2 * h1) * (2 * w1) * 64 * 81
    conv2 = 2.0 * (2 * t2) * (2 * h2) * (2 * w2) * 128 * 1728
    conv3 = 2.0 * t2 * h2 * w2 * 256 * 3456
    head = 2.0 * 256 * classes
    weights = 4.0 * (64 * 81 + 64 + 128 * 1728 + 128 + 256 * 3456 + 256 + classes * 257)
    return {"conv1": conv1, "conv2": conv2, "conv3": conv3, "head": head, "clip": conv1 + conv2 + conv3 + head,
            "pool1": (frames, h1, w1), "pool2": (t2, h2, w2), "clip_bytes": 4.0 * 3 * frames * h * w, "weight_bytes": weights,
            "act1_bytes": 4.0 * frames * h1 * w1 * 64, "act2_bytes": 4.0 * t2 * h2 * w2 * 128}


def pack_cnn3d(net, half: bool = False) -> Dict[str, np.ndarray]:
    """The ``rva_cnn3d_weights`` arrays of a :class:`temporal.Cnn3dNet` (``N.Cnn3dWeights.NAMES`` order), contiguous fp32, each
    Conv3d with its BatchNorm folded in float64 and rounded once, in the layouts the kernels read:

      * ``conv1_w`` ``[64, 3, 3, 3, 3]`` = ``[co, ci, kt, ky, kx]`` (the module's own layout: the VALU kernel keeps a channel's
        81 taps in registers in this order);
      * ``conv2_w`` ``[128, 27, 64]`` and ``conv3_w`` ``[256, 27, 128]`` = ``[co, tap, ci]`` with ``tap = (kt*3 + ky)*3 + kx``
        (channels innermost, as the channels-last activations: a lane's MFMA operands are contiguous float4 reads);
      * biases ``[64]`` / ``[128]`` / ``[256]``, ``head_w`` ``[classes, 256]``, ``head_b`` ``[classes]``.

    ``half=True`` (the fp16 plan): each convolution weight is folded in float64, rounded once to fp16 and widened to fp32 --
    the values ``rva_cnn3d_f16_plan_create`` then converts exactly; a value beyond fp16 raises ``ValueError``.  Biases and the head
    stay fp32."""
    seq, fc = getattr(net, "conv3d", None), getattr(net, "fc", None)
    ok = isinstance(seq, torch.nn.Sequential) and len(seq) == 12 and isinstance(fc, torch.nn.Linear)
    if ok:
        for i, (cin, cout) in zip((0, 4, 8), ((3, 64), (64, 128), (128, 256))):
            c, bn = seq[i], seq[i + 1]
            ok = ok and isinstance(c, torch.nn.Conv3d) and isinstance(bn, torch.nn.BatchNorm3d) and \
                (c.in_channels, c.out_channels) == (cin, cout) and c.kernel_size == (3, 3, 3) and c.stride == (1, 1, 1) and \
                c.padding == (1, 1, 1) and c.dilation == (1, 1, 1) and c.groups == 1
        p1, p2 = seq[3], seq[7]
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3  # noqa: E731
        ok = ok and isinstance(p1, torch.nn.MaxPool3d) and pair(p1.kernel_size) == (1, 2, 2) and pair(p1.stride) == (1, 2, 2) and \
            isinstance(p2, torch.nn.MaxPool3d) and pair(p2.kernel_size) == (2, 2, 2) and pair(p2.stride) == (2, 2, 2) and \
            pair(p1.padding) == (0, 0, 0) and pair(p2.padding) == (0, 0, 0) and not p1.ceil_mode and not p2.ceil_mode and \
            isinstance(seq[11], torch.nn.AdaptiveAvgPool3d) and fc.in_features == 256
    if not ok:
        raise ValueError("pack_cnn3d: not the Cnn3dNet architecture")
    fold = (lambda i, what: _fold_f16(seq[i], seq[i + 1], what)) if half else (lambda i, what: _fold(seq[i], seq[i + 1]))  # noqa: E731
    c1w, c1b = fold(0, "conv1_w")
    c2w, c2b = fold(4, "conv2_w")
    c3w, c3b = fold(8, "conv3_w")
    taps_last = lambda w: w.reshape(w.shape[0], w.shape[1], 27).transpose(0, 2, 1)  # noqa: E731  [co,ci,27] -> [co,27,ci]
    bias = fc.bias.detach().float().cpu().numpy() if fc.bias is not None else np.zeros(fc.out_features, np.float32)
    out = {"conv1_w": c1w, "conv1_b": c1b, "conv2_w": taps_last(c2w), "conv2_b": c2b, "conv3_w": taps_last(c3w), "conv3_b": c3b,
           "head_w": fc.weight.detach().float().cpu().numpy(), "head_b": bias}
    return {n: np.ascontiguousarray(out[n], dtype=np.float32) for n in N.Cnn3dWeights.NAMES}


class Fused3dCnn(_ClipPlan):
    """One ``rva_cnn3d_plan``: the fp32 clip network of ``net`` (a :class:`temporal.Cnn3dNet`) for clips of ``frames`` frames at
    ``hw``, up to ``max_clips`` clips per call.  Same surface as :class:`FusedCnnLstm` (``max_clips``, ``T``, ``classes``,
    ``logits``, ``run``, ``post``, ``__call__``).  No host synchronisation and no allocation after construction (capturable)."""

    ABI = "rva_cnn3d_plan"
    HALF = False                              # pack_cnn3d(half=...): the precision of the convolution weights

    def __init__(self, net, hw: Tuple[int, int], frames: int, max_clips: int, ctx: Optional[N.Context] = None,
                 device: Optional[torch.device] = None):
        packed = pack_cnn3d(net, half=self.HALF)                    # a wrong architecture is refused before the device is touched
        self._open(hw, frames, max_clips, net.fc.out_features, ctx, device)
        self._create(N.Cnn3dDesc(self.H, self.W, self.T, self.classes, self.max_clips), N.Cnn3dWeights, packed)
        p1, p2, tiles, nl = (C.c_int32 * 3)(), (C.c_int32 * 3)(), (C.c_int32 * 3)(), C.c_int32()
        self.ctx.check(self._fn("info")(self.handle, p1, p2, tiles, C.byref(nl)), f"{self.ABI}_info")
        self.pool1, self.pool2, self.tiles, self.n_launches = tuple(p1), tuple(p2), tuple(tiles), nl.value

    def stage(self, name: str, n_clips: int) -> torch.Tensor:
        """A copy of one intermediate tensor of the last :meth:`run` (of at least ``n_clips`` clips, on the current stream), in
        the layout ``rva_cnn3d_plan_stage`` documents (include/rva.h): ``"act1"`` ``[n, T, H1, W1, 64]``, ``"act2"``
        ``[n, T2*H2*W2, 128]``, ``"partial"`` ``[n, conv3_tiles, 256]``, ``"feat"`` ``[n, 256]``.  A read-only tap for tests and
        tools."""
        n = int(n_clips)
        stages = {"act1": (0, (n, *self.pool1, 64)), "act2": (1, (n, int(np.prod(self.pool2)), 128)),
                  "partial": (2, (n, self.tiles[2], 256)), "feat": (3, (n, 256))}
        return self._tap(stages, name, n)

    def __call__(self, clips: torch.Tensor) -> torch.Tensor:
        """``Cnn3dNet.forward`` of clips ``[B, 3, T, H, W]`` fp32: a fresh ``[B, classes]`` tensor.  The permute to frames
        ``[B, T, 3, H, W]`` is for this (test) path only: the detector's ring holds planar frames already."""
        b = int(clips.shape[0])
        if tuple(clips.shape[1:]) != (3, self.T, self.H, self.W):
            raise ValueError(f"clips must be [B, 3, {self.T}, {self.H}, {self.W}], got {tuple(clips.shape)}")
        return self._run_frames(clips.permute(0, 2, 1, 3, 4).contiguous(), b)


class Fused3dCnnF16(Fused3dCnn):
    """One ``rva_cnn3d_f16_plan``: the network of :class:`Fused3dCnn` for ``half: true`` -- fp16 frames, fp16 convolution weights
    (``net``'s fp32 parameters folded in float64 and rounded once) and fp16 stored activations on the fp16 MFMA, every sum in
    fp32, fp32 logits.  Same surface: ``run`` takes an fp16 ring, ``stage`` returns ``act1`` / ``act2`` as fp16 tensors."""

    ABI = "rva_cnn3d_f16_plan"
    HALF = True
    RING_DTYPE = torch.float16
    TAP_DTYPES = {"act1": torch.float16, "act2": torch.float16}

    def __call__(self, clips: torch.Tensor) -> torch.Tensor:
        """``Cnn3dNet.forward`` of clips ``[B, 3, T, H, W]`` of fp16, or of fp32 that is rounded to fp16 here: a fresh fp32
        ``[B, classes]`` tensor."""
        return super().__call__(clips.to(torch.float16))


def fired_tables(fired: Sequence, cols: Sequence[int], ring_columns: int, rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """Host tables of one tick: frame indices into ``ring.view(-1, 3, H, W)`` (clip-major) and the ``[rows, 3]`` result-row
    table (clip or -1, width, height).  ``fired``: ``(row, ring slots of the clip, (h, w))`` as ``stage_pre`` lists them."""
    idx = np.array([sl * ring_columns + cols[row] for row, slots, _ in fired for sl in slots], dtype=np.int32)
    tab = np.zeros((rows, 3), dtype=np.int32)
    tab[:, 0] = -1
    for clip, (row, _, hw) in enumerate(fired):
        tab[row] = (clip, hw[1], hw[0])
    return idx, tab
