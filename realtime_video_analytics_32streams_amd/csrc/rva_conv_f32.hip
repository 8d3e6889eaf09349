// fp32 YOLOv8 primitives: the arithmetic of the reference's default precision (`half: false`, detector.py:248-251: an fp32 ONNX
// Runtime graph) on hand-written kernels, everything fp32 in and out -- activations, weights, bias, accumulation, SiLU, head.
//
// Convolution: NHWC implicit GEMM on the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32: bit-for-bit a k-ordered fmaf chain, no
// reduced-precision shortcut).  Rows of the GEMM = output pixels, columns = output channels, K = k*k*Cin.  Every variant (tile
// shape) and every batch size runs the SAME reduction for an output element: the order rva_mfma_f32.h defines, with chunks of
// CK = 32 channels when Cin % 32 == 0, else 16.  Bias, SiLU (x / (1 + expf(-x))) and the residual follow in that order.
// Results are therefore bit-identical across variants, batch sizes and launch orders.  A lane reads only the channels
// [0, Cin) of its input slice (Cin % 16 == 0): nothing next door is ever multiplied, not even by a zero weight.
#include "rva_internal.h"
#include "rva_mfma_f32.h"

namespace {

struct ConvF32Args {
    const float *in; int ldi;
    const float *w;                  // [Cout][k*k][Cin]
    const float *bias;               // [Cout] or null
    float *out; int ldo;
    const float *res; int ldr;       // residual (added after SiLU) or null
    int B, H, W, Ho, Wo, Cin, Cout, k, stride, pad, act;
    long M;                          // B * Ho * Wo
};

// MT x NT tiles of 32 x 32 per wave, WM x WN waves per 256-thread block
template <int MT, int NT, int WM, int WN, int CK>
__global__ void __launch_bounds__(256) k_conv_f32(ConvF32Args a)
{
    static_assert(WM * WN == 4, "four waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int r = lane & 31, h = lane >> 5;
    const long m0 = ((long)blockIdx.x * WM + wm) * (32 * MT);
    const int n0 = (blockIdx.y * WN + wn) * (32 * NT);
    const int kk = a.k * a.k;

    int pn[MT], py[MT], px[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        long p = m0 + mt * 32 + r;
        pv[mt] = p < a.M;
        if (!pv[mt]) p = 0;
        px[mt] = (int)(p % a.Wo);
        py[mt] = (int)((p / a.Wo) % a.Ho);
        pn[mt] = (int)(p / ((long)a.Wo * a.Ho));
    }
    const float *wrow[NT];
    bool wv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + nt * 32 + r;
        wv[nt] = co < a.Cout;
        wrow[nt] = a.w + (size_t)(wv[nt] ? co : 0) * kk * a.Cin + (CK / 2) * h;
    }
    f32x16 acc[MT][NT] = {};
    for (int tap = 0; tap < kk; ++tap) {
        const int ky = tap / a.k, kx = tap - ky * a.k;
        const float *arow[MT];
        bool av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int iy = py[mt] * a.stride + ky - a.pad, ix = px[mt] * a.stride + kx - a.pad;
            av[mt] = pv[mt] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            arow[mt] = a.in + ((size_t)((long)pn[mt] * a.H + (av[mt] ? iy : 0)) * a.W + (av[mt] ? ix : 0)) * a.ldi + (CK / 2) * h;
        }
        const size_t wtap = (size_t)tap * a.Cin;
        for (int c = 0; c < a.Cin; c += CK) f32_chunk<MT, NT, CK>(acc, arow, av, c, wrow, wv, wtap + c);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + nt * 32 + r;
        if (co >= a.Cout) continue;
        const float bias = a.bias ? a.bias[co] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long p = m0 + mt * 32 + f32_cd_row(i, h);
                if (p >= a.M) continue;
                float v = acc[mt][nt][i] + bias;
                if (a.act) v = v / (1.f + expf(-v));
                if (a.res) v = v + a.res[(size_t)p * a.ldr + co];
                a.out[(size_t)p * a.ldo + co] = v;
            }
        }
    }
}

// Variants: (MT, NT, WM, WN) -> block tile (32 MT WM) pixels x (32 NT WN) channels.  Listed here; 0 = heuristic.
struct F32Variant { int mt, nt, wm, wn; };
constexpr F32Variant kF32Variants[] = {
    {2, 2, 4, 1},    // 1: 256 x 64
    {2, 2, 2, 2},    // 2: 128 x 128
    {1, 2, 4, 1},    // 3: 128 x 64
    {2, 1, 4, 1},    // 4: 256 x 32
    {1, 1, 4, 1},    // 5: 128 x 32
    {1, 2, 2, 2},    // 6: 64 x 128
};
constexpr int kNumF32Variants = (int)(sizeof kF32Variants / sizeof kF32Variants[0]);

template <int CK>
void launch_conv_f32(int v, dim3 g, hipStream_t st, const ConvF32Args &a)
{
    switch (v) {
    case 1: k_conv_f32<2, 2, 4, 1, CK><<<g, 256, 0, st>>>(a); break;
    case 2: k_conv_f32<2, 2, 2, 2, CK><<<g, 256, 0, st>>>(a); break;
    case 3: k_conv_f32<1, 2, 4, 1, CK><<<g, 256, 0, st>>>(a); break;
    case 4: k_conv_f32<2, 1, 4, 1, CK><<<g, 256, 0, st>>>(a); break;
    case 5: k_conv_f32<1, 1, 4, 1, CK><<<g, 256, 0, st>>>(a); break;
    default: k_conv_f32<1, 2, 2, 2, CK><<<g, 256, 0, st>>>(a); break;
    }
}

dim3 conv_f32_grid(int v, long M, int Cout)
{
    const F32Variant &t = kF32Variants[v - 1];
    return dim3((unsigned)((M + 32L * t.mt * t.wm - 1) / (32L * t.mt * t.wm)), (unsigned)rva_ceil_div(Cout, 32 * t.nt * t.wn));
}

// variant 0: the largest tile that still gives every CU two blocks; narrow layers (Cout <= 32) keep NT = 1
int conv_f32_heuristic(long M, int Cout, int num_cus)
{
    const int order_wide[] = {2, 1, 3, 6, 5}, order_narrow[] = {4, 5};
    const int *order = Cout <= 32 ? order_narrow : order_wide;
    const int n = Cout <= 32 ? 2 : 5;
    const long want = 2L * (num_cus > 0 ? num_cus : 256);
    for (int i = 0; i < n; ++i) {
        const int v = order[i];
        if (kF32Variants[v - 1].nt * kF32Variants[v - 1].wn * 32 > 2 * rva_ceil_div(Cout, 32) * 32) continue;   // mostly empty columns
        const dim3 g = conv_f32_grid(v, M, Cout);
        if ((long)g.x * g.y >= want) return v;
    }
    return order[n - 1];
}

// ---------------------------------------------------------------------------------------------------
// Stem: 3x3 stride 2 pad 1 from the planar fp32 [B,3,H,W] tensor K1 writes, VALU.  weights = the checkpoint's [Cout][3][3][3]
// (27 taps in (c, ky, kx) order, summed in that order with fmaf), NHWC out.  Thread = (output pixel, 4 channels).
__global__ void __launch_bounds__(256) k_stem_f32(const float *in, const float *w, const float *bias, float *out, int ldo, int B,
                                                  int H, int W, int Ho, int Wo, int Cout)
{
    const int nq = Cout >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * Ho * Wo * nq) return;
    const int q = (int)(idx % nq);
    const long pix = idx / nq;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
    float x[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = oy * 2 + ky - 1, ix = ox * 2 + kx - 1;
                x[c * 9 + ky * 3 + kx] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                                             ? in[((size_t)(b * 3 + c) * H + iy) * W + ix] : 0.f;
            }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int co = q * 4 + j;
        const float *wr = w + (size_t)co * 27;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 27; ++t) s = fmaf(x[t], wr[t], s);
        s = s + (bias ? bias[co] : 0.f);
        o[j] = s / (1.f + expf(-s));
    }
    *reinterpret_cast<float4 *>(out + (size_t)pix * ldo + q * 4) = make_float4(o[0], o[1], o[2], o[3]);
}

// 5x5 stride-1 pad-2 max pool over a channel slice (-inf padding): thread = (pixel, 4 channels)
__global__ void __launch_bounds__(256) k_maxpool5_f32(const float *in, int ldi, float *out, int ldo, int B, int H, int W, int C)
{
    const int cg = C >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * H * W * cg) return;
    const int g = (int)(idx % cg);
    const long pix = idx / cg;
    const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy;
        if ((unsigned)yy >= (unsigned)H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx;
            if ((unsigned)xx >= (unsigned)W) continue;
            const float4 v = *reinterpret_cast<const float4 *>(in + ((size_t)(b * H + yy) * W + xx) * ldi + g * 4);
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    }
    *reinterpret_cast<float4 *>(out + (size_t)pix * ldo + g * 4) = m;
}

// nearest 2x upsample into a channel slice: out pixel (y, x) <- in pixel (y/2, x/2); thread = (out pixel, 4 channels)
__global__ void __launch_bounds__(256) k_upsample2_f32(const float *in, int ldi, float *out, int ldo, int B, int H, int W, int C)
{
    const int cg = C >> 2, Ho = H * 2, Wo = W * 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * Ho * Wo * cg) return;
    const int g = (int)(idx % cg);
    const long pix = idx / cg;
    const int x = (int)(pix % Wo), y = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
    *reinterpret_cast<float4 *>(out + (size_t)pix * ldo + g * 4) =
        *reinterpret_cast<const float4 *>(in + ((size_t)(b * H + (y >> 1)) * W + (x >> 1)) * ldi + g * 4);
}

// Detect head of one level, the module's formula (yolov8.py DetectHead.forward) in fp32: DFL softmax (max-subtracted, expf) ->
// expectation -> x1y1 = anchor - lt, x2y2 = anchor + rb -> xywh = ((x1y1 + x2y2) / 2, x2y2 - x1y1) * stride; classes: sigmoid.
// out[B, 4+nc, A] at anchor offset a0.  Thread = anchor.
__global__ void __launch_bounds__(256) k_head_f32(const float *box, int ldb, const float *cls, int ldc, float *out, int h, int w,
                                                  int nc, int A, int a0, float stride)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= h * w) return;
    const size_t pix = (size_t)b * h * w + i;
    const float *bp = box + pix * ldb;
    float d[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float v[16], mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 16; t += 4) {
            const float4 q = *reinterpret_cast<const float4 *>(bp + s * 16 + t);
            v[t] = q.x; v[t + 1] = q.y; v[t + 2] = q.z; v[t + 3] = q.w;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) mx = fmaxf(mx, v[t]);
        float se = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) { v[t] = expf(v[t] - mx); se = se + v[t]; }
        float e = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) e = e + (v[t] / se) * (float)t;
        d[s] = e;
    }
    const float ax = (float)(i % w) + 0.5f, ay = (float)(i / w) + 0.5f;
    const float x1 = ax - d[0], y1 = ay - d[1], x2 = ax + d[2], y2 = ay + d[3];
    float *o = out + (size_t)b * (4 + nc) * A + a0 + i;
    o[0] = (x1 + x2) / 2.f * stride;
    o[(size_t)A] = (y1 + y2) / 2.f * stride;
    o[(size_t)2 * A] = (x2 - x1) * stride;
    o[(size_t)3 * A] = (y2 - y1) * stride;
    const float *cp = cls + pix * ldc;
    for (int c = 0; c < nc; ++c) o[(size_t)(4 + c) * A] = 1.f / (1.f + expf(-cp[c]));
}

bool aligned16(const void *p) { return p && ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int rva_conv_f32_num_variants(void) { return kNumF32Variants; }

int rva_conv2d_nhwc_f32_v(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias, void *out, int ldo,
                          const void *residual, int ldr, int batch, int H, int W, int Cin, int Cout, int ksize, int stride, int act,
                          int variant, rva_stream_t stream_)
{
    if (!ctx) return RVA_ERR_ARG;
    if (!aligned16(in) || !aligned16(weights) || !out || batch <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin % 16 || Cout <= 0 ||
        (ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || ldi % 4 || ldi < Cin || ldo < Cout ||
        (residual && ldr < Cout) || variant < 0 || variant > kNumF32Variants)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_conv2d_nhwc_f32_v: bad argument (Cin %% 16 == 0, ksize 1/3, stride 1/2, ldi %% 4 == 0, "
                        "16-byte aligned input and weights, variant 0..%d)", kNumF32Variants);
    ConvF32Args a{};
    a.in = (const float *)in; a.ldi = ldi; a.w = (const float *)weights; a.bias = bias; a.out = (float *)out; a.ldo = ldo;
    a.res = (const float *)residual; a.ldr = ldr;
    a.B = batch; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.k = ksize; a.stride = stride; a.pad = ksize / 2; a.act = act;
    a.Ho = (H + 2 * a.pad - ksize) / stride + 1; a.Wo = (W + 2 * a.pad - ksize) / stride + 1;
    a.M = (long)batch * a.Ho * a.Wo;
    const int v = variant ? variant : conv_f32_heuristic(a.M, Cout, rva_num_cus(ctx));
    const dim3 g = conv_f32_grid(v, a.M, Cout);
    if (Cin % 32 == 0) launch_conv_f32<32>(v, g, (hipStream_t)stream_, a);
    else launch_conv_f32<16>(v, g, (hipStream_t)stream_, a);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_stem_conv_f32(rva_ctx *ctx, const void *in_planar, const void *weights, const float *bias, void *out, int ldo, int batch,
                      int H, int W, int Cout, rva_stream_t stream_)
{
    if (!ctx || !in_planar || !weights || !aligned16(out) || batch <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout % 4 || ldo % 4 || ldo < Cout)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_stem_conv_f32: bad argument");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long n = (long)batch * Ho * Wo * (Cout / 4);
    k_stem_f32<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>((const float *)in_planar, (const float *)weights, bias,
                                                                               (float *)out, ldo, batch, H, W, Ho, Wo, Cout);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_maxpool5_nhwc_f32(rva_ctx *ctx, const void *in, int ldi, void *out, int ldo, int batch, int H, int W, int C, rva_stream_t stream_)
{
    if (!ctx || !aligned16(in) || !aligned16(out) || C <= 0 || C % 4 || ldi % 4 || ldo % 4)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_maxpool5_nhwc_f32: bad argument");
    const long n = (long)batch * H * W * (C / 4);
    k_maxpool5_f32<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>((const float *)in, ldi, (float *)out, ldo, batch, H, W, C);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_upsample2x_nhwc_f32(rva_ctx *ctx, const void *in, int ldi, void *out, int ldo, int batch, int H, int W, int C, rva_stream_t stream_)
{
    if (!ctx || !aligned16(in) || !aligned16(out) || C <= 0 || C % 4 || ldi % 4 || ldo % 4)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_upsample2x_nhwc_f32: bad argument");
    const long n = (long)batch * H * 2 * W * 2 * (C / 4);
    k_upsample2_f32<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>((const float *)in, ldi, (float *)out, ldo, batch, H, W, C);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_yolo_head_f32(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc, void *out, int batch, int h, int w,
                      int nc, int anchors_total, int anchor_offset, float stride, rva_stream_t stream_)
{
    if (!ctx || !aligned16(box_logits) || !cls_logits || !out || ldb % 4 || ldb < 64 || ldc < nc || nc <= 0 || batch <= 0 || h <= 0 ||
        w <= 0 || anchor_offset < 0 || anchor_offset + h * w > anchors_total)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head_f32: bad argument");
    k_head_f32<<<dim3(rva_ceil_div(h * w, 256), batch), 256, 0, (hipStream_t)stream_>>>((const float *)box_logits, ldb,
                                                                                       (const float *)cls_logits, ldc, (float *)out, h, w,
                                                                                       nc, anchors_total, anchor_offset, stride);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

}  // extern "C"
