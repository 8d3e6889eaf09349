"""Fused YOLOv8 execution plan: the tuner and a thin caller of ``rva_yolov8_plan_*`` (include/rva.h).

The plan itself -- weight packing, the NHWC fp16 activation buffers, the static list of launches (one per Conv-BN-SiLU;
``torch.cat`` / ``chunk`` / upsample never materialise), the fork / join of the detect branches -- is built and replayed in C
(``csrc/rva_plan.hip``): one ABI call per forward pass.  What stays here:

  * handing the seeded / loaded ``yolov8.YoloV8`` module (BatchNorm folded) to ``rva_yolov8_plan_create`` as a list of
    convolutions in module order;
  * the per-layer kernel selection: every applicable variant of every convolution step is timed on the plan's own buffers
    through ``rva_yolov8_plan_launch_tunable`` and the choice fixed with ``rva_yolov8_plan_set_variant``; the selection is
    persisted per (device, library build, plan shape);
  * the result tensors (a pipelined caller alternates several).

Output: the same ``[B, 4+nc, A]`` fp16 tensor the torch module returns, so everything downstream (K2/K3/K4) and every parity
test is unchanged.  ``precision="fp32"`` builds the same plan in the reference's own precision (``RVA_PLAN_F32``: fp32 input,
activations, weights and ``[B, 4+nc, A]`` fp32 output; kernels of ``csrc/rva_conv_f32.hip``, bit-identical across kernel variants).
``box_rows="fp32"`` (fp16 plans, opt-in; ``RVA_PLAN_BOX_F32``) makes the head kernels also store the four box rows as an fp32 side
tensor ``boxes32[B, 4, A]`` of the same output slot -- one allocation with the head tensor, which is still written in full and is
bit-identical to the default plan's; ``ops.postprocess(..., boxes=plan.boxes32)`` reads its boxes from it.
``static_rows=(top, bottom)`` (fp16 plans) is the caller's promise that the input rows outside that window -- a letterbox border --
hold the same bytes on every run: after one priming run over all rows the early layers launch only the output rows that depend on
the window (``rva_yolov8_plan_set_static_rows``, include/rva.h); results are bit-identical.
``batch`` is the plan's capacity: a call takes ``[n,3,H,W]`` with ``1 <= n <= batch`` and runs the leading ``n`` images of every
buffer (``rva_yolov8_plan_run_n``) with the kernels of a full run, so ``out[:n]`` is bit-identical to the same images of a full run
and ``out[n:]`` is not touched.
No host synchronisation and no allocation after construction: a whole tick can be captured into a hipGraph.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native as N
from . import ops
from .yolov8 import C2f, ConvBnAct, YoloV8


_LIB_DIGEST: Optional[str] = None


def _lib_digest() -> str:
    """sha256 of librva.so: a rebuilt library never inherits another build's kernel selection."""
    global _LIB_DIGEST
    if _LIB_DIGEST is None:
        _LIB_DIGEST = hashlib.sha256(N.LIB_PATH.read_bytes()).hexdigest()
    return _LIB_DIGEST


def _tuning_dir():
    d = os.environ.get("RVA_TUNE_CACHE_DIR")
    return Path(d) if d else Path(os.environ.get("XDG_CACHE_HOME", str(Path.home() / ".cache"))) / "rva_amd" / "autotune"


def module_order_convs(net: YoloV8) -> list:
    """The convolutions of a fused ``YoloV8`` in the module order ``rva_yolov8_plan_create`` consumes (include/rva.h)."""
    def c2f(m: C2f):
        out = [m.cv1, m.cv2]
        for b in m.m:
            out += [b.cv1, b.cv2]
        return out
    mods = [net.b0, net.b1, *c2f(net.b2), net.b3, *c2f(net.b4), net.b5, *c2f(net.b6), net.b7, *c2f(net.b8), net.b9.cv1, net.b9.cv2,
            *c2f(net.h12), *c2f(net.h15), net.h16, *c2f(net.h18), net.h19, *c2f(net.h21)]
    for branch in (net.detect.box, net.detect.cls):
        for seq in branch:
            mods += [seq[0], seq[1], seq[2]]
    return [m.conv if isinstance(m, ConvBnAct) else m for m in mods]


class _VariantCell:
    """``state["variant"]`` of one tunable step, stored in the C plan."""

    __slots__ = ("eng", "idx")

    def __init__(self, eng, idx):
        self.eng, self.idx = eng, idx

    def __getitem__(self, key):
        assert key == "variant"
        return int(self.eng.L.rva_yolov8_plan_get_variant(self.eng.handle, self.idx))

    def __setitem__(self, key, value):
        assert key == "variant"
        self.eng.ctx.check(self.eng.L.rva_yolov8_plan_set_variant(self.eng.handle, self.idx, int(value)), "rva_yolov8_plan_set_variant")


class FusedYoloV8:
    HEAD_ROWS_EXTRA = 4                   # rows of the head tensor beside the classes: xywh
    ARCH_KEY = b""                        # joins the tuning key where it is not empty (YOLOv8 keys stay as they were)

    def __init__(self, net: YoloV8, batch: int, hw: Tuple[int, int] = (640, 640), device: Optional[torch.device] = None,
                 ctx: Optional[N.Context] = None, autotune: bool = True, tune_overlap: int = 1, precision: str = "fp16",
                 box_rows: str = "fp16", static_rows: Optional[Tuple[int, int]] = None):
        if precision not in ("fp16", "fp32"):
            raise ValueError(f"precision must be 'fp16' or 'fp32', not {precision!r}")
        if box_rows not in ("fp16", "fp32"):
            raise ValueError(f"box_rows must be 'fp16' or 'fp32', not {box_rows!r}")
        if box_rows == "fp32" and precision == "fp32":
            raise ValueError("box_rows='fp32' belongs to the fp16 plan: the output of precision='fp32' is fp32 already")
        self.box_rows = box_rows
        self.precision = precision
        self.f32 = precision == "fp32"
        self.tune_overlap = int(tune_overlap)
        self.ctx = ctx or ops.context()
        self.dev = device or torch.device("cuda", self.ctx.device)
        self.B, self.H, self.W = batch, hw[0], hw[1]
        self.n = batch                     # images of the last run (or of the tensor a caller announced): what result() hands out
        assert hw[0] % 32 == 0 and hw[1] % 32 == 0
        net = net.fuse()
        self.nc = net.nc
        self.L = N.lib()
        convs = self._module_order(net)
        keep, arr = [], (N.ConvWeights * len(convs))()
        for i, c in enumerate(convs):
            w = np.ascontiguousarray(c.weight.detach().float().cpu().numpy())
            b = None if c.bias is None else np.ascontiguousarray(c.bias.detach().float().cpu().numpy())
            keep += [w, b]
            arr[i].weight = w.ctypes.data_as(C.POINTER(C.c_float))
            arr[i].bias = b.ctypes.data_as(C.POINTER(C.c_float)) if b is not None else None
            arr[i].cout, arr[i].cin, arr[i].k, arr[i].stride = int(w.shape[0]), int(w.shape[1]), int(w.shape[2]), int(c.stride[0])
        d, create = self._descriptor(net, batch, hw, len(convs))
        d.flags = (N.RVA_PLAN_NO_STEM2 if os.environ.get("RVA_NO_STEM2", "0") == "1" else 0) | \
                  (N.RVA_PLAN_NO_CIN_PAD if os.environ.get("RVA_NO_CIN_PAD", "0") == "1" else 0) | \
                  (0 if self._use_pair32() else N.RVA_PLAN_NO_PAIR32) | \
                  (N.RVA_PLAN_F32 if self.f32 else 0) | (N.RVA_PLAN_BOX_F32 if box_rows == "fp32" else 0)
        h = C.c_void_p()
        with torch.cuda.device(self.dev):
            self.ctx.check(getattr(self.L, create)(self.ctx.handle, C.byref(d), arr, C.byref(h)), create)
        self.handle = h
        del keep
        # row windows: set before the tuner runs, so that it times the windowed launches -- what will run
        self.static_rows = (0, self.H)
        self.rows_epoch = 0                # bumped by every set_static_rows: a hipGraph recorded with windows is good for one epoch
        if static_rows is not None and tuple(static_rows) != (0, self.H) and os.environ.get("RVA_PLAN_NO_STATIC_ROWS") != "1":
            self.ctx.check(self.L.rva_yolov8_plan_set_static_rows(h, int(static_rows[0]), int(static_rows[1])), "rva_yolov8_plan_set_static_rows")
            self.static_rows = (int(static_rows[0]), int(static_rows[1]))
        info = [C.c_int32() for _ in range(5)]
        self.ctx.check(self.L.rva_yolov8_plan_info(h, *[C.byref(v) for v in info]), "rva_yolov8_plan_info")
        self.A, rows, self._n_steps, n_tun, self.quiet_step = (int(v.value) for v in info)
        assert rows == self.HEAD_ROWS_EXTRA + self.nc
        self.dtype = torch.float32 if self.f32 else torch.float16
        self.boxes32: Optional[torch.Tensor] = None       # box_rows="fp32": the side tensor of the current output slot
        self._boxes = {}
        if box_rows == "fp32":
            total, off = C.c_int64(), C.c_int64()
            self.ctx.check(self.L.rva_yolov8_plan_output_layout(h, C.byref(total), C.byref(off)), "rva_yolov8_plan_output_layout")
            self._out_layout = (int(total.value), int(off.value))
            self.out, self.boxes32 = self._alloc_split()
            self._boxes[0] = self.boxes32
        else:
            self.out = torch.empty((batch, rows, self.A), dtype=self.dtype, device=self.dev)
        self._outs = {0: self.out}
        self.fused_stem = isinstance(d, (N.YoloV8Desc, N.Yolo11Desc)) and not self.f32 and not (d.flags & N.RVA_PLAN_NO_STEM2) and tuple(d.widths[:2]) == (32, 64)
        # (launch(stream, variant) -> rc, state["variant"], "Cin->Cout kKsS HxW") per convolution step, as the tuner and the tools use them
        self._n_tunable = n_tun
        self._read_tunables()
        self._side = None                   # two side streams for the detect branches, created on first use
        self._forks = bool(self.fused_head_lanes())
        self.concurrent_heads = os.environ.get("RVA_SERIAL_HEADS") != "1"      # A/B switch for measurements
        if autotune:
            self.autotune()

    @staticmethod
    def _module_order(net) -> list:
        return module_order_convs(net)

    @staticmethod
    def _descriptor(net, batch: int, hw: Tuple[int, int], n_convs: int):
        """The plan descriptor of ``net`` (flags left to the caller) and the name of the create entry point that takes it."""
        d = N.YoloV8Desc()
        d.batch, d.height, d.width = batch, hw[0], hw[1]
        d.widths[:] = [net.b0.conv.out_channels, net.b1.conv.out_channels, net.b3.conv.out_channels, net.b5.conv.out_channels,
                       net.b7.conv.out_channels]
        d.depth_backbone[:] = [len(net.b2.m), len(net.b4.m), len(net.b6.m), len(net.b8.m)]
        d.depth_head = len(net.h12.m)
        assert len(net.h15.m) == len(net.h18.m) == len(net.h21.m) == d.depth_head
        d.nc, d.reg_max, d.n_convs = net.nc, net.detect.reg_max, n_convs
        return d, "rva_yolov8_plan_create"

    def _read_tunables(self) -> None:
        self._tunable = []
        buf = C.create_string_buffer(96)
        for i in range(self._n_tunable):
            self.ctx.check(self.L.rva_yolov8_plan_tunable_desc(self.handle, i, buf, 96), "rva_yolov8_plan_tunable_desc")

            def launch(stream, variant, i=i):
                return self.L.rva_yolov8_plan_launch_tunable(self.handle, i, variant, C.c_void_p(self.out.data_ptr()), stream)
            self._tunable.append((launch, _VariantCell(self, i), buf.value.decode()))

    def set_static_rows(self, top: int, bottom: int) -> None:
        """Input rows outside ``[top, bottom)`` hold the same bytes on every run from now on (``(0, H)``: no such rows).  The plan
        is unprimed afterwards: its next complete run covers all rows.  The kernel selection stays as it is (a selection made
        for other windows is still correct: a kernel that cannot restrict rows runs them all)."""
        self.ctx.check(self.L.rva_yolov8_plan_set_static_rows(self.handle, int(top), int(bottom)), "rva_yolov8_plan_set_static_rows")
        if os.environ.get("RVA_PLAN_NO_STATIC_ROWS") == "1":
            return                         # A/B switch: the library made the call a no-op
        self.static_rows = (int(top), int(bottom))
        self.rows_epoch += 1
        self._read_tunables()              # the descriptions carry the windows

    @property
    def primed_images(self) -> int:
        """Leading images whose buffers hold a whole run's rows (``rva_yolov8_plan_primed_images``; never mirrored here)."""
        return int(self.L.rva_yolov8_plan_primed_images(self.handle))

    @property
    def primed(self) -> bool:
        """Whether a run of the last run's ``n`` images launches row windows: a complete eager run has covered all their rows."""
        return self.primed_images >= self.n

    def step_rows(self, step: int) -> Tuple[int, int]:
        y0, y1 = C.c_int32(), C.c_int32()
        self.ctx.check(self.L.rva_yolov8_plan_step_rows(self.handle, int(step), C.byref(y0), C.byref(y1)), "rva_yolov8_plan_step_rows")
        return int(y0.value), int(y1.value)

    def step_desc(self, step: int) -> str:
        """What step ``step`` of the launch list is (``rva_yolov8_plan_step_desc``): a convolution's tunable description, else
        the kernel and its shape."""
        buf = C.create_string_buffer(96)
        self.ctx.check(self.L.rva_yolov8_plan_step_desc(self.handle, int(step), buf, 96), "rva_yolov8_plan_step_desc")
        return buf.value.decode()

    def _alloc_split(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """One allocation in the plan's output layout: the fp16 head, then ``boxes32`` at the offset the plan reports."""
        total, off = self._out_layout
        rows = self.HEAD_ROWS_EXTRA + self.nc
        buf = torch.empty((total,), dtype=torch.uint8, device=self.dev)
        head = buf[:self.B * rows * self.A * 2].view(torch.float16).view(self.B, rows, self.A)
        boxes = buf[off:off + self.B * 4 * self.A * 4].view(torch.float32).view(self.B, 4, self.A)
        return head, boxes

    def fused_head_lanes(self) -> bool:
        """Whether the plan has detect branches that may run on side streams (head decode fused into the branches, or an fp32
        plan, whose per-level head launches ride on the branches' lanes)."""
        return self.f32 or any(d.startswith("head1:") for _, _, d in self._tunable)

    def __del__(self):  # best effort
        try:
            if getattr(self, "handle", None):
                self.L.rva_yolov8_plan_destroy(self.handle)
                self.handle = None
        except Exception:  # noqa: BLE001
            pass

    # -- per-layer kernel selection ---------------------------------------------------------------------
    # -- persisted kernel selection -----------------------------------------------------------------------
    def _tuning_key(self) -> str:
        """What a kernel selection depends on: the device, the library build, the layer shapes of the plan (batch included)
        and the switches that change how the selection is made."""
        h = hashlib.sha256()
        h.update(torch.cuda.get_device_name(self.dev).encode())
        h.update(_lib_digest().encode())
        h.update(repr((self.B, self.H, self.W, [d for _, _, d in self._tunable])).encode())
        h.update(b"per-layer times; in-plan pass opt-in, three overlapping passes")
        # "" where RVA_TUNE_IN_PLAN, _OVERLAP, _TOP, _WITHIN and RVA_HEAD_SPLIT were hashed: retired switches, and old keys stay valid
        skip, no_stem2, no_cin_pad = (os.environ.get(k, "") for k in ("RVA_SKIP_VARIANTS", "RVA_NO_STEM2", "RVA_NO_CIN_PAD"))
        h.update(repr([skip, "", "", "", "", no_stem2, "", no_cin_pad]).encode())
        h.update(repr(int(os.environ.get("RVA_TUNE_LAYER_OVERLAP", getattr(self, "tune_overlap", 1)))).encode())
        if getattr(self, "f32", False):
            h.update(b"precision fp32")                 # fp16 keys stay as they were: existing caches remain valid
        if self.ARCH_KEY:
            h.update(self.ARCH_KEY)
        return h.hexdigest()[:24]

    def _load_tuning(self) -> bool:
        f = _tuning_dir() / f"{self._tuning_key()}.json"
        try:
            rec = json.loads(f.read_text())
            picks = rec["variants"]
            if len(picks) != len(self._tunable) or any(d != pd for (_, _, d), (pd, _) in zip(self._tunable, picks)):
                return False
        except (OSError, ValueError, KeyError, TypeError):
            return False
        try:
            for (_, state, _), (_, v) in zip(self._tunable, picks):
                state["variant"] = int(v)          # the plan checks the variant number against this build (a stale or edited file)
        except RuntimeError:
            for _, state, _ in self._tunable:
                state["variant"] = 0
            return False
        self.tuning = [tuple(t) for t in rec.get("tuning", [])]
        self.tuning_source = str(f)
        return True

    def _store_tuning(self) -> None:
        d = _tuning_dir()
        try:
            d.mkdir(parents=True, exist_ok=True)
            tmp = d / f".{self._tuning_key()}.{os.getpid()}.tmp"
            tmp.write_text(json.dumps({"device": torch.cuda.get_device_name(self.dev), "batch": self.B, "hw": [self.H, self.W],
                                       "variants": [[desc, st["variant"]] for _, st, desc in self._tunable],
                                       "tuning": [list(t) for t in self.tuning]}))
            os.replace(tmp, d / f"{self._tuning_key()}.json")            # atomic: concurrent ranks write the same content
        except OSError:
            pass                                                        # a read-only cache directory costs start-up time only

    def autotune(self, reps: int = 5) -> None:
        """Time every applicable conv kernel variant on each layer's real shape (buffers hold whatever they
        hold: timing only) and keep the fastest.  All variants compute the same sums in fp32 with the same
        per-chunk order of K, so the choice does not change results beyond fp32 summation order.  The selection is
        persisted per (device, library build, plan shape): a later process takes it over instead of timing again
        (``RVA_TUNE_CACHE=0`` disables, ``RVA_TUNE_CACHE_DIR`` moves it)."""
        self.tuning_source = "measured"
        use_cache = os.environ.get("RVA_TUNE_CACHE", "1") == "1"
        if use_cache and self._load_tuning():
            return
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.tuning = []
        self._n_variants = int(N.lib().rva_conv_num_variants())
        skip = {int(v) for v in os.environ.get("RVA_SKIP_VARIANTS", "").replace(",", " ").split()}      # tuning aid: same-box A/B of kernel families
        cache = {}
        # What a launch costs a pipeline with several ticks in flight is not its time alone on the chip but the share of the chip it
        # holds for that time: a one-workgroup-per-CU kernel (120-150 KB of LDS) that is 15 % faster alone than a two-per-CU one
        # leaves no room for the other chains' kernels while it runs.  tune_overlap = n >= 2 times every candidate as n launches
        # side by side on the chains' own streams (behind a spin kernel, so that the host's launch rate stays out of the
        # measurement) and keeps the variant with the lowest time PER LAUNCH; 1 = the launch alone (lowest latency: one tick at a
        # time, the paced operating point).  PipelinedTicks sets it to its depth; RVA_TUNE_LAYER_OVERLAP overrides.
        n_over = int(os.environ.get("RVA_TUNE_LAYER_OVERLAP", getattr(self, "tune_overlap", 1)))
        lanes = ops.chain_streams(self.dev, n_over) if n_over >= 2 else []
        spin = int(os.environ.get("RVA_TUNE_SPIN_CYCLES", "400000"))       # ~0.2 ms: every stream's launches are queued before any starts

        def time_variant(variant) -> float:
            torch.cuda.synchronize()
            if not lanes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    launch(stream, variant)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps * 1e3
            evs = []
            for st in lanes:
                with torch.cuda.stream(st):
                    torch.cuda._sleep(spin)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    sp = C.c_void_p(st.cuda_stream)
                    for _ in range(reps):
                        launch(sp, variant)
                    b.record()
                    evs.append((a, b))
            torch.cuda.synchronize()
            # from the first stream's start to the last stream's end (the spins end within microseconds of each other)
            first = evs[0][0]
            return max(first.elapsed_time(b) for _, b in evs) / (reps * len(lanes)) * 1e3
        for launch, state, desc in self._tunable:
            if desc in cache:
                state["variant"] = cache[desc][0]
                continue
            best = (0, float("inf"))
            for variant in range(1, self._n_variants + 1):
                if variant in skip or launch(stream, variant) != N.RVA_OK:
                    continue
                us = time_variant(variant)
                if us < best[1]:
                    best = (variant, us)
            state["variant"] = best[0]
            cache[desc] = best
            self.tuning.append((desc, best[0], round(best[1], 1)))
        if use_cache:
            self._store_tuning()

    def copy_tuning(self, other: "FusedYoloV8") -> None:
        """Take over the kernel selection of a plan built from the same network and batch shape."""
        assert len(self._tunable) == len(other._tunable) and self.precision == other.precision      # (either box_rows: same selection)
        for (_, mine, d1), (_, theirs, d2) in zip(self._tunable, other._tunable):
            assert d1 == d2
            mine["variant"] = theirs["variant"]
        self.tuning = list(getattr(other, "tuning", []))
        self.tuning_source = "copied from the first slot's plan"

    # -- run ------------------------------------------------------------------------------------------
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """``x``: fp16 (fp32 for an fp32 plan) planar ``[n,3,H,W]`` contiguous (what K1 writes), ``1 <= n <= B``.  Returns
        ``out[:n]``: ``[n, 4+nc, A]`` of the plan's precision, image for image the bits of a full run.  One ABI call."""
        assert x.is_cuda and x.dtype == self.dtype and x.is_contiguous() and x.dim() == 4 and tuple(x.shape[1:]) == (3, self.H, self.W)
        n = int(x.shape[0])
        assert 1 <= n <= self.B, f"{n} images on a plan of capacity {self.B}"
        self.n = n
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        xin, out = C.c_void_p(x.data_ptr()), C.c_void_p(self.out.data_ptr())
        if self.concurrent_heads and self._forks:
            # fork / join over events inside the plan: works eagerly and inside a stream capture
            if self._side is None:
                self._side = (torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev))
            self.ctx.check(self.L.rva_yolov8_plan_run_lanes_n(self.handle, xin, out, n, stream, C.c_void_p(self._side[0].cuda_stream),
                                                              C.c_void_p(self._side[1].cuda_stream)), "rva_yolov8_plan_run_lanes_n")
            return self._head()
        self.ctx.check(self.L.rva_yolov8_plan_run_n(self.handle, xin, out, n, stream), "rva_yolov8_plan_run_n")
        return self._head()

    def _head(self) -> torch.Tensor:
        """The head tensor of the last run's images in the current output slot (the slot itself for a full run)."""
        return self.out if self.n == self.B else self.out[:self.n]

    def use_output(self, index: int) -> torch.Tensor:
        """Select which result tensor the head kernels write (``index`` 0 is the one allocated at construction, others are
        allocated on first use).  A pipelined caller alternates two per tick (and uses a pair per frame group), so the
        post-process of tick k can still read its head tensor on another HIP stream while the network of tick k+1 runs."""
        if index not in self._outs:
            if self.box_rows == "fp32":
                self._outs[index], self._boxes[index] = self._alloc_split()
            else:
                self._outs[index] = torch.empty_like(self._outs[0])
        self.out = self._outs[index]
        self.boxes32 = self._boxes.get(index)
        return self.out

    def result(self):
        """What a caller hands to the post-process for the current output slot: the head tensor of the last run's ``n`` images, or
        with ``box_rows="fp32"`` an ``ops.SplitHead`` of it and of the same images of its side tensor."""
        if self.boxes32 is None:
            return self._head()
        return ops.SplitHead(self._head(), self.boxes32 if self.n == self.B else self.boxes32[:self.n])

    def _use_pair32(self) -> bool:
        """The 32-channel C2f bottleneck (YOLOv8s at 160 x 160) as ONE launch with the intermediate in LDS (rva_c2f_pair32_f16) or as
        two convolution launches.  Fused, a forward pass alone is 2.2 % shorter (1.749 against 1.787 ms, bit-identical output) -- less
        memory traffic in a bandwidth-bound stage -- but it recomputes the intermediate's halo (+30 % SiLUs and MFMAs in that stage),
        and with four forward passes side by side, where instruction issue and not bandwidth is what is short, the pipeline loses
        0.5 % (22.36-22.41 k against 22.47-22.55 k frames/s, same box, three alternating pairs).  So: fused for a plan that serves one
        tick at a time (tune_overlap <= 1: `TickPipeline.tick()`, the per-frame API, depth-1 runners), two launches for a plan that
        serves overlapping ticks.  ``RVA_PAIR32=1 / 0`` forces either."""
        env = os.environ.get("RVA_PAIR32")
        if env in ("0", "1"):
            return env == "1"
        return int(os.environ.get("RVA_TUNE_LAYER_OVERLAP", self.tune_overlap)) <= 1

    @property
    def n_launches(self) -> int:
        return self._n_steps


def module_order_convs_v5(net) -> list:
    """The convolutions of a fused ``yolov5.YoloV5`` in the module order ``rva_yolov5_plan_create`` consumes (include/rva.h)."""
    def c3(m):
        out = [m.cv1, m.cv2, m.cv3]
        for b in m.m:
            out += [b.cv1, b.cv2]
        return out
    mods = [net.b0, net.b1, *c3(net.b2), net.b3, *c3(net.b4), net.b5, *c3(net.b6), net.b7, *c3(net.b8), net.b9.cv1, net.b9.cv2,
            net.h10, *c3(net.h13), net.h14, *c3(net.h17), net.h18, *c3(net.h20), net.h21, *c3(net.h23), *net.detect.m]
    return [m.conv if isinstance(m, ConvBnAct) else m for m in mods]


class FusedYoloV5(FusedYoloV8):
    """The fused fp16 plan of a ``yolov5.YoloV5`` (``rva_yolov5_plan_create``): the same plan object, tuner and surface as
    ``FusedYoloV8`` -- ``__call__``, ``result()``, ``use_output``, ``n``, ``set_static_rows``, ``copy_tuning``, ``n_launches``,
    ``boxes32`` -- with the head tensor ``[B, 5 + nc, A]`` (anchor axis contiguous; the transpose of the module's output).
    There is no fp32 YOLOv5 plan: ``precision="fp32"`` is a ``ValueError``."""

    HEAD_ROWS_EXTRA = 5                   # xywh + objectness
    ARCH_KEY = b"arch yolov5"

    def __init__(self, net, batch: int, hw: Tuple[int, int] = (640, 640), **kw):
        if kw.get("precision", "fp16") != "fp16":
            raise ValueError("there is no fp32 YOLOv5 plan: FusedYoloV5 runs precision='fp16' (half: true)")
        super().__init__(net, batch, hw, **kw)

    @staticmethod
    def _module_order(net) -> list:
        return module_order_convs_v5(net)

    @staticmethod
    def _descriptor(net, batch: int, hw: Tuple[int, int], n_convs: int):
        d = N.YoloV5Desc()
        d.batch, d.height, d.width = batch, hw[0], hw[1]
        d.widths[:] = [net.b0.conv.out_channels, net.b1.conv.out_channels, net.b3.conv.out_channels, net.b5.conv.out_channels,
                       net.b7.conv.out_channels]
        d.depth_backbone[:] = [len(net.b2.m), len(net.b4.m), len(net.b6.m), len(net.b8.m)]
        d.depth_head = len(net.h13.m)
        assert len(net.h17.m) == len(net.h20.m) == len(net.h23.m) == d.depth_head
        d.nc, d.n_convs = net.nc, n_convs
        d.anchors[:] = [float(v) for v in net.detect.anchors_px.detach().float().cpu().flatten().tolist()]
        return d, "rva_yolov5_plan_create"


def module_order_convs_11(net) -> list:
    """The convolutions of a fused ``yolo11.Yolo11`` in the module order ``rva_yolo11_plan_create`` consumes (include/rva.h).
    The depthwise ones (``groups == channels``) have weights ``[C, 1, 3, 3]`` and travel as ``cin = 1``."""
    from .yolo11 import C3k

    def bottleneck(b):
        return [b.cv1, b.cv2]

    def c3k2(m):
        out = [m.cv1, m.cv2]
        for b in m.m:
            if isinstance(b, C3k):
                out += [b.cv1, b.cv2, b.cv3]
                for bb in b.m:
                    out += bottleneck(bb)
            else:
                out += bottleneck(b)
        return out

    def c2psa(m):
        out = [m.cv1, m.cv2]
        for b in m.m:
            out += [b.attn.qkv, b.attn.proj, b.attn.pe, b.ffn[0], b.ffn[1]]
        return out
    mods = [net.l0, net.l1, *c3k2(net.l2), net.l3, *c3k2(net.l4), net.l5, *c3k2(net.l6), net.l7, *c3k2(net.l8), net.l9.cv1, net.l9.cv2,
            *c2psa(net.l10), *c3k2(net.l13), *c3k2(net.l16), net.l17, *c3k2(net.l19), net.l20, *c3k2(net.l22)]
    for seq in net.detect.box:
        mods += [seq[0], seq[1], seq[2]]
    for seq in net.detect.cls:
        mods += [seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2]]
    return [m.conv if isinstance(m, ConvBnAct) else m for m in mods]


class FusedYolo11(FusedYoloV8):
    """The fused fp16 plan of a ``yolo11.Yolo11`` (``rva_yolo11_plan_create``): the same plan object, tuner and surface as
    ``FusedYoloV8``, and the same head tensor ``[B, 4 + nc, A]``.  The depthwise convolutions and the attention of C2PSA are fixed
    kernels (``rva_dwconv3x3_nhwc_f16``, ``rva_psa_attention_f16``): the tuner sees the ordinary convolutions only, the qkv / proj /
    ffn 1x1 among them.  The detect branches run in line (no side lanes).  There is no fp32 YOLO11 plan: ``precision="fp32"`` is a
    ``ValueError``."""

    HEAD_ROWS_EXTRA = 4
    ARCH_KEY = b"arch yolo11"

    def __init__(self, net, batch: int, hw: Tuple[int, int] = (640, 640), **kw):
        if kw.get("precision", "fp16") != "fp16":
            raise ValueError("there is no fp32 YOLO11 plan: FusedYolo11 runs precision='fp16' (half: true)")
        super().__init__(net, batch, hw, **kw)

    @staticmethod
    def _module_order(net) -> list:
        return module_order_convs_11(net)

    @staticmethod
    def _descriptor(net, batch: int, hw: Tuple[int, int], n_convs: int):
        d = N.Yolo11Desc()
        d.batch, d.height, d.width = batch, hw[0], hw[1]
        d.widths[:] = [net.l0.conv.out_channels, net.l1.conv.out_channels, net.l3.conv.out_channels, net.l5.conv.out_channels,
                       net.l7.conv.out_channels]
        blocks = (net.l2, net.l4, net.l6, net.l8, net.l13, net.l16, net.l19, net.l22)
        d.repeats[:] = [len(m.m) for m in blocks]
        d.c3k[:] = [int(m.c3k) for m in blocks]
        d.psa_blocks, d.psa_heads = len(net.l10.m), net.l10.m[0].attn.num_heads
        d.nc, d.n_convs = net.nc, n_convs
        return d, "rva_yolo11_plan_create"

    def fused_head_lanes(self) -> bool:
        return False                      # the plan has no fork points: rva_yolov8_plan_run_lanes_n is _run_n
