"""Float64 references and derived rounding bounds for every stage of the two fp32 clip plans (csrc/rva_clip.hip,
csrc/rva_clip3d.hip), shared by tests/test_clip_stages_host.py (CPU: the bounds see the bugs) and the GPU stage tests.

Every stage is computed in float64 from the tensor the kernel under test itself read (the tap of the stage before it), so a
bound covers the rounding of ONE kernel.  All bounds but the LSTM's are derived, with u = 2**-24 (fp32 unit roundoff):

  * an fp32 dot product of n terms plus a bias, in any order, fma or MFMA, errs by at most (n + 2) u (sum |w_i x_i| + |b|) to
    first order: ``tol = (n + 2) u (conv(|x|, |w|) + |b|)``, evaluated per element in float64;
  * ReLU and max are 1-Lipschitz, so a pooled value errs by at most the largest bound in its window;
  * a tile partial (sum of <= 256 ReLU'd values, as 2 x 16 per lane, 2 lane halves, 4 waves) errs by at most
    ``sum_p tol_p + 258 u sum_p v_p``;
  * the mean (tiles - 1 additions and a division): ``(tiles + 1) u sum_k |partial_k| / P``;
  * the LSTM's ``expf`` cannot be bounded from the source: its bound is 64 x the error of torch's own fp32 LSTM against
    float64 on the same input (``lstm_e_ref``), floored at 1e-6.

Layouts are those of ``rva_cnnlstm_plan_stage`` / ``rva_cnn3d_plan_stage`` (include/rva.h)."""
import numpy as np
import torch
import torch.nn.functional as F

from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.clip_plan import conv_out, pack_cnn3d, pack_cnn_lstm
from realtime_video_analytics_32streams_amd.temporal import Cnn3dNet, CnnLstmNet

U = 2.0 ** -24
TILE = 256                                  # positions of a conv2 (CNN-LSTM) / conv3 (3D) block
LSTM_FACTOR, LSTM_FLOOR = 64.0, 1e-6

# (H, W, T, hidden, classes, n_clips, cap)
LSTM_SHAPES = [(2, 2, 1, 5, 3, 1, 1), (40, 56, 4, 48, 24, 2, 2), (30, 34, 2, 16, 5, 1, 1), (64, 64, 2, 16, 5, 17, 17),
               (67, 131, 3, 130, 10, 9, 12)]
# (T, H, W, classes, n_clips, cap)
C3D_SHAPES = [(2, 4, 4, 3, 1, 1), (7, 25, 41, 10, 2, 2), (4, 36, 68, 10, 3, 4)]


def shape_id(s):
    return "x".join(str(v) for v in s)


def f64(a):
    return (a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).double()


def lstm_case(shape):
    """Seeded module, its packed fp32 weights as float64 tensors, and clips ``[n, T, 3, H, W]`` fp32 of one CNN-LSTM shape."""
    H, W, T, hidden, classes, n, _ = shape
    seed = 100 + LSTM_SHAPES.index(tuple(shape))
    net = synth.seeded_module(lambda: CnnLstmNet(classes, hidden), seed)
    return net, {k: f64(v) for k, v in pack_cnn_lstm(net).items()}, synth.seeded_clip((n, T, 3, H, W), seed + 50)


def c3d_case(shape):
    """Seeded module (the last BatchNorm's bias raised by 1), packed weights (float64; conv2 / conv3 back in the module's ``[co,
    ci, 3, 3, 3]``) and frames ``[n, T, 3, H, W]`` fp32 (the ring's layout) of one 3D-CNN shape."""
    T, H, W, classes, n, _ = shape
    seed = 200 + C3D_SHAPES.index(tuple(shape))
    net = synth.seeded_module(lambda: Cnn3dNet(classes), seed)
    # conv3's outputs one unit up: with the seeded statistics a ReLU'd output is 1.5 % of its sum of |products|, and one position
    # left out of a tile sum of 180 would be 2 x the tile's rounding bound; with the offset it is 6 x (the host test's rule is 4 x)
    net.conv3d[9].bias.data += 1.0
    p = {k: f64(v) for k, v in pack_cnn3d(net).items()}
    for k in ("conv2_w", "conv3_w"):
        w = p[k]
        p[k] = w.permute(0, 2, 1).reshape(w.shape[0], w.shape[2], 3, 3, 3).contiguous()
    return net, p, synth.seeded_clip((n, T, 3, H, W), seed + 50)


# ---------------------------------------------------------------------------------------------------------------------
# generic pieces
def conv_bound(conv, x, w, b, n, **kw):
    """(conv(x, w) + b, its fp32 bound (n + 2) u (conv(|x|, |w|) + |b|)), both float64."""
    x, w, b = f64(x), f64(w), f64(b)
    return conv(x, w, b, **kw), (n + 2) * U * conv(x.abs(), w.abs(), b.abs(), **kw)


def linear(x, w, b, n):
    """(x . w^T + b, bound) of a dot product of n terms per output."""
    x, w, b = f64(x), f64(w), f64(b)
    return x @ w.T + b, (n + 2) * U * (x.abs() @ w.abs().T + b.abs())


def tile_partial(v, tol):
    """``v``, ``tol`` = ``[F, C, P]`` ReLU'd map and its bound, P linear in raster order -> (partial ``[F, tiles, C]``, bound)."""
    P = v.shape[2]
    parts, tols = [], []
    for k in range(0, P, TILE):
        s = v[:, :, k:k + TILE].sum(2)
        parts.append(s)
        tols.append(tol[:, :, k:k + TILE].sum(2) + 258 * U * s)
    return torch.stack(parts, 1), torch.stack(tols, 1)


def tile_partial_in_kernel_order(y, dtype=np.float32):
    """The tile sums of f32_tile_sum (csrc/rva_mfma_f32.h) from the map before the ReLU, ``y [F, P, C]`` -> ``[F, tiles, C]``, every
    operation in ``dtype``: v = max(y, 0); per tile of 256 positions, per wave (64 positions from m0 = 256 tile + 64 wave) and
    lane half h a sum from zero over positions m0 + 32 mt + (i & 3) + 8 (i >> 2) + 4 h for mt = 0, 1 then i = 0 .. 15, positions
    >= P skipped; then halves 0 + 1; then waves 0 .. 3 added in order to zero."""
    v = np.maximum(np.asarray(y, dtype=dtype), dtype(0))
    F_, P, C_ = v.shape
    out = np.zeros((F_, -(-P // TILE), C_), dtype=dtype)
    for tile in range(out.shape[1]):
        total = np.zeros((F_, C_), dtype=dtype)
        for wave in range(4):
            m0 = tile * TILE + wave * 64
            halves = []
            for h in range(2):
                s = np.zeros((F_, C_), dtype=dtype)
                for mt in range(2):
                    for i in range(16):
                        p = m0 + mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h
                        if p < P:
                            s = s + v[:, p]
                halves.append(s)
            total = total + (halves[0] + halves[1])
        out[:, tile] = total
    assert out.dtype == dtype
    return out


def feat_from_partial(partial, P):
    """``[F, tiles, C]`` tile sums -> (mean ``[F, C]``, bound)."""
    partial = f64(partial)
    return partial.sum(1) / P, (partial.shape[1] + 1) * U * partial.abs().sum(1) / P


def ratio(got, ref, tol):
    """max |got - ref| / tol over the tensor (an element whose bound is 0 must be exact)."""
    err = (f64(got) - ref).abs()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(r.max()), float(err.max())


def report(shape, stage, got, ref, tol, out=None, limit=1.0):
    """Print ``observed / bound`` of one stage; append the stage to ``out`` if it is over ``limit``."""
    assert tuple(got.shape) == tuple(ref.shape), (stage, tuple(got.shape), tuple(ref.shape))
    r, e = ratio(got, ref, tol)
    print(f"{shape_id(shape)} {stage}: max err {e:.3e}, max bound {float(tol.max()):.3e}, observed / bound = {r:.3f}")
    if out is not None and not r <= limit:
        out.append(f"{stage}: observed / bound = {r:.3f} (max err {e:.3e})")
    return r


# ---------------------------------------------------------------------------------------------------------------------
# CNN-LSTM
def stem_conv(frames, p):
    """frames ``[F, 3, H, W]`` -> (conv1 with BN folded ``[F, 64, Hc, Wc]`` before ReLU, bound); n = 147."""
    return conv_bound(F.conv2d, frames, p["conv1_w"], p["conv1_b"], 147, stride=2, padding=3)


def stem_pool(y, tol):
    """ReLU + MaxPool(3, 2, 1) -> (pooled ``[F, Hp, Wp, 64]``, bound)."""
    return (F.max_pool2d(y.relu(), 3, 2, 1).permute(0, 2, 3, 1).contiguous(),
            F.max_pool2d(tol, 3, 2, 1).permute(0, 2, 3, 1).contiguous())


def conv2_map(pooled, p):
    """pooled tap ``[F, Hp, Wp, 64]`` -> (conv2 with BN folded ``[F, 128, Hp, Wp]`` before ReLU, bound); n = 576."""
    return conv_bound(F.conv2d, f64(pooled).permute(0, 3, 1, 2), p["conv2_w"], p["conv2_b"], 576, padding=1)


def partial_from_map(y, tol):
    """Pre-ReLU map ``[F, C, *spatial]`` -> (tile partials ``[F, tiles, C]``, bound)."""
    return tile_partial(y.relu().flatten(2), tol.flatten(2))


def gx_from_feat(feat, p, n, T):
    g, t = linear(feat, p["w_ih1"], p["b1"], 128)
    return g.view(n, T, -1), t.view(n, T, -1)


def lstm(gx, p, mut=None, dtype=torch.float64):
    """The 2-layer LSTM from layer 1's input projection ``gx [n, T, 4h]`` -> (h1, h2) ``[T, n, h]``, gates i, f, g, o.
    ``mut``: ``"c0_from_8"`` (previous cell state read as 0 for clips >= 8) or ``"l2_next"`` (layer 2 reads h1 of the next
    step, clamped at the end) -- the bug classes of k_clip_lstm, for the host test."""
    gx = f64(gx).to(dtype)
    whh1, wih2, whh2, b2 = (p[k].to(dtype) for k in ("w_hh1", "w_ih2", "w_hh2", "b2"))
    n, T, G4 = gx.shape
    h = G4 // 4

    def cell(pre, c):
        i, f, g, o = pre.view(n, 4, h).unbind(1)
        if mut == "c0_from_8":
            c = c.clone()
            c[8:] = 0
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c), c

    z = torch.zeros((n, h), dtype=dtype)
    h1, hp, c = [], z, z
    for t in range(T):
        hp, c = cell(gx[:, t] + hp @ whh1.T, c)
        h1.append(hp)
    h2, hp, c = [], z, z
    for t in range(T):
        x = h1[min(t + 1, T - 1)] if mut == "l2_next" else h1[t]
        hp, c = cell(x @ wih2.T + hp @ whh2.T + b2, c)
        h2.append(hp)
    return torch.stack(h1), torch.stack(h2)


def torch_lstm(feat, p, n, T, dtype):
    """torch.nn.LSTM (the module's own operator) with the packed weights on ``feat [n*T, 128]`` -> (h1, h2) ``[T, n, h]``."""
    h = p["w_hh1"].shape[1]
    out = []
    x = f64(feat).view(n, T, 128).to(dtype)
    with torch.no_grad():
        for wi, wh, b in ((p["w_ih1"], p["w_hh1"], p["b1"]), (p["w_ih2"], p["w_hh2"], p["b2"])):
            m = torch.nn.LSTM(wi.shape[1], h, 1, batch_first=True).to(dtype)
            m.weight_ih_l0.copy_(wi); m.weight_hh_l0.copy_(wh); m.bias_ih_l0.copy_(b); m.bias_hh_l0.zero_()
            x = m(x)[0]
            out.append(x.transpose(0, 1).double())
    return out


def lstm_e_ref(feat, p, n, T):
    """Max error of torch's fp32 LSTM against its float64 copy on the same features, over both layers and every step."""
    a, b = torch_lstm(feat, p, n, T, torch.float32), torch_lstm(feat, p, n, T, torch.float64)
    return max(float((x - y).abs().max()) for x, y in zip(a, b))


def lstm_bound(e_ref):
    return max(LSTM_FACTOR * e_ref, LSTM_FLOOR)


def head(x, p):
    return linear(x, p["head_w"], p["head_b"], p["head_w"].shape[1])


def lstm_refs(taps, clips, p, shape):
    """``taps``: name -> fp32 tensor in the tap layout (pooled, partial, feat, gx, h1, h2).  Returns name -> (ref, tol) with
    each stage computed from the tap before it; ``e_ref`` and the LSTM bound ride along under ``"_lstm"``.  ``taps = None``
    chains the references themselves, each rounded once to fp32 (what an exact kernel would leave in the workspace)."""
    H, W, T, hidden, classes, n, _ = shape
    out = {}
    tap = (lambda k: taps[k]) if taps is not None else (lambda k: out[k][0].float())
    y, t = stem_conv(f64(clips).flatten(0, 1), p)
    out["pooled"] = stem_pool(y, t)
    y, t = conv2_map(tap("pooled"), p)
    out["partial"] = partial_from_map(y, t)
    out["feat"] = feat_from_partial(tap("partial"), y.shape[2] * y.shape[3])
    out["gx"] = gx_from_feat(tap("feat"), p, n, T)
    e_ref = lstm_e_ref(tap("feat"), p, n, T)
    h1, h2 = lstm(tap("gx"), p)
    b = torch.full_like(h1, lstm_bound(e_ref))
    out["h1"], out["h2"] = (h1, b), (h2, b)
    out["logits"] = head(f64(tap("h2"))[T - 1], p)
    out["_lstm"] = (e_ref, lstm_bound(e_ref))
    return out


def pooled_hw(H, W):
    return conv_out(conv_out(H, 7, 2, 3), 3, 2, 1), conv_out(conv_out(W, 7, 2, 3), 3, 2, 1)


# ---------------------------------------------------------------------------------------------------------------------
# 3D-CNN
def c3d_conv1(frames, p):
    """frames ``[n, T, 3, H, W]`` -> (conv1 with BN folded ``[n, 64, T, H, W]`` before ReLU / pool, bound); n = 81."""
    return conv_bound(F.conv3d, f64(frames).permute(0, 2, 1, 3, 4), p["conv1_w"], p["conv1_b"], 81, padding=1)


def c3d_pool(y, tol, k):
    """ReLU + floor MaxPool3d(k) -> channels-last (act, bound)."""
    return (F.max_pool3d(y.relu(), k, k).permute(0, 2, 3, 4, 1).contiguous(), F.max_pool3d(tol, k, k).permute(0, 2, 3, 4, 1).contiguous())


def c3d_conv2(act1, p):
    """act1 tap ``[n, T, H1, W1, 64]`` -> (conv2 ``[n, 128, T, H1, W1]`` before ReLU / pool, bound); n = 1728."""
    return conv_bound(F.conv3d, f64(act1).permute(0, 4, 1, 2, 3), p["conv2_w"], p["conv2_b"], 1728, padding=1)


def c3d_conv3(act2, p, thw):
    """act2 tap ``[n, T2*H2*W2, 128]`` -> (conv3 ``[n, 256, T2, H2, W2]`` before ReLU, bound); n = 3456."""
    a = f64(act2)
    return conv_bound(F.conv3d, a.view(a.shape[0], *thw, 128).permute(0, 4, 1, 2, 3), p["conv3_w"], p["conv3_b"], 3456, padding=1)


def c3d_refs(taps, frames, p, shape):
    """As ``lstm_refs`` for the 3D plan: act1, act2, partial, feat, logits."""
    T, H, W = shape[:3]
    thw = (T // 2, H // 4, W // 4)
    out = {}
    tap = (lambda k: taps[k]) if taps is not None else (lambda k: out[k][0].float())
    out["act1"] = c3d_pool(*c3d_conv1(frames, p), (1, 2, 2))
    a, t = c3d_pool(*c3d_conv2(tap("act1"), p), (2, 2, 2))
    out["act2"] = (a.flatten(1, 3), t.flatten(1, 3))
    out["partial"] = partial_from_map(*c3d_conv3(tap("act2"), p, thw))
    out["feat"] = feat_from_partial(tap("partial"), thw[0] * thw[1] * thw[2])
    out["logits"] = linear(tap("feat"), p["head_w"], p["head_b"], 256)
    return out
