// The 3D-CNN clip network of rva_clip3d.hip for `half: true` (engine "clip3d-f16"): the same network, launches, block and wave
// decomposition, with fp16 frames, fp16 convolution weights and fp16 stored activations, and every sum in fp32:
//
//   * input: the detector's ring of planar fp16 frames [3][H][W], read through the device table of frame indices;
//   * weights: BatchNorm folded by the caller in float64; rva_cnn3d_f16_plan_create rounds each convolution weight once to fp16
//     (round to nearest even; a value that does not stay finite is refused).  Biases, head weight and head bias stay fp32;
//   * every convolution sum accumulates in fp32 in ONE fixed order (rva_mfma_f16.h for conv2 / conv3, an fmaf chain for conv1):
//     the fp32 plan's reproducibility contract holds unchanged;
//   * epilogues: max of the raw fp32 sums, + bias, ReLU, then ONE rounding to fp16 for act1 / act2; conv3's tile partials, the
//     mean, the head and the logits are fp32 (the shared rva_clip_* launches).
//
//   K_conv1  as k_c3d_conv1: the fp16 frames are widened to fp32 on the way into LDS (exact) and the weights are the fp16-rounded
//            values held as fp32, so the fmaf chain over (ci, kt, ky, kx) adds exact products.  Frame rows are read element by
//            element: nothing is assumed about the alignment of a row (odd widths).  Writes fp16 [T][H/2][W/2][64].
//   K_conv2  27 taps x 64 channels on v_mfma_f32_32x32x16_f16; pool + bias + ReLU in the epilogue.  Writes fp16 [T/2][H/4][W/4][128].
//   K_conv3  27 taps x 128 channels, same core; f32_tile_sum.  Writes fp32 tile partials.
//            Both stage a step's weights (one tap x 64 channels of the block's 128 output channels) through LDS once per block
//            (f16_conv_taps_wlds); RVA_C3D16_WLDS=0 at plan creation selects the straight port in which every wave loads its own
//            (f16_conv_taps; bit 0 = conv2, bit 1 = conv3).  Same reduction order: the two are bit-identical.
//   K_mean / K_head / K_post: the kernels of rva_clip.hip.
#include "rva_internal.h"
#include "rva_mfma_f16.h"

#include <cmath>

namespace {

constexpr int C1 = 64, C2 = 128, C3 = 256;                 // widths of the architecture
constexpr int TAPS = 27;
constexpr int PT = 8;                                      // pooled tile (PT x PT) of K_conv1
constexpr int IT = 2 * PT + 2;                             // input rows / columns of that tile (18)
constexpr int ITW = IT + 2;                                // padded LDS row (20)
constexpr int CONV1_THREADS = 256;
constexpr int MT = 2, NT = 4;                              // 32x32 MFMA tiles of a wave: 64 positions x 128 channels
constexpr int GROUPS = 32;                                 // pool groups (of 8 conv positions) of a K_conv2 block
constexpr int MAX_CLASSES = 16384;

// ---------------------------------------------------------------------------------------------------
// K_conv1.  Thread = output channel (tid & 63) x a wave-uniform pooled position; the input reads are LDS broadcasts and each thread
// keeps its 81 weights in registers.  Sum of a conv output: fmaf chain from 0 over (ci, kt, ky, kx) in order; then max of the
// four, + bias, ReLU, one rounding to fp16.
__global__ void __launch_bounds__(CONV1_THREADS) k_c3d16_conv1(const _Float16 *ring, const int32_t *frame_index, const float *w1,
                                                               const float *b1, _Float16 *act1, int T, int H, int W, int H1, int W1,
                                                               int tiles_x)
{
    __shared__ float xin[3 * 3 * IT * ITW];                // [kt][ci][IT][ITW]
    const int f = blockIdx.y, t = f % T;
    const int py0 = (blockIdx.x / tiles_x) * PT, px0 = (blockIdx.x % tiles_x) * PT;
    const int iy0 = 2 * py0 - 1, ix0 = 2 * px0 - 1;
    for (int kt = 0; kt < 3; ++kt) {
        const int tt = t + kt - 1;
        const bool tv = (unsigned)tt < (unsigned)T;       // block-uniform
        const _Float16 *img = tv ? ring + (size_t)frame_index[f + kt - 1] * 3 * H * W : ring;
        for (int i = threadIdx.x; i < 3 * IT * IT; i += CONV1_THREADS) {
            const int c = i / (IT * IT), rr = (i / IT) % IT, q = i % IT;
            const int iy = iy0 + rr, ix = ix0 + q;
            xin[((kt * 3 + c) * IT + rr) * ITW + q] =
                (tv && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) ? (float)img[((size_t)c * H + iy) * W + ix] : 0.f;
        }
    }
    const int co = threadIdx.x & (C1 - 1), grp = threadIdx.x >> 6;
    float w[3 * TAPS];
#pragma unroll
    for (int k = 0; k < 3 * TAPS; ++k) w[k] = w1[co * 3 * TAPS + k];
    const float bias = b1[co];
    __syncthreads();
    for (int p = grp; p < PT * PT; p += CONV1_THREADS / 64) {
        const int ly = p / PT, lx = p % PT, py = py0 + ly, px = px0 + lx;
        if (py >= H1 || px >= W1) continue;                // wave-uniform
        float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int kt = 0; kt < 3; ++kt) {
                const float *xr = xin + ((kt * 3 + c) * IT + 2 * ly) * ITW + 2 * lx;
                float x[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) x[a][b] = xr[a * ITW + b];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float wv = w[((c * 3 + kt) * 3 + ky) * 3 + kx];
                        s00 = fmaf(x[ky][kx], wv, s00);
                        s01 = fmaf(x[ky][kx + 1], wv, s01);
                        s10 = fmaf(x[ky + 1][kx], wv, s10);
                        s11 = fmaf(x[ky + 1][kx + 1], wv, s11);
                    }
            }
        const float m = fmaxf(fmaxf(s00, s01), fmaxf(s10, s11));
        act1[(((size_t)f * H1 + py) * W1 + px) * C1 + co] = (_Float16)fmaxf(m + bias, 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------
// K_conv2.  The decomposition and the epilogue of k_c3d_conv2: block = 32 pool groups (linear over [T2][H2][W2]) of one clip x all
// 128 channels; wave = 8 groups = 64 conv positions; row m of a wave's 64 = group m >> 3, position (dt, dy, dx) = bits 2, 1, 0 of
// m & 7.  Registers 4j .. 4j+3 of a lane are half a pool group and the other lane half holds the rest.
template <bool WLDS>
__global__ void __launch_bounds__(256) k_c3d16_conv2(const _Float16 *act1, const _Float16 *w2, const float *b2, _Float16 *act2, int T,
                                                     int H1, int W1, int T2, int H2, int W2)
{
    const int clip = blockIdx.y, tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int NG = T2 * H2 * W2;
    const int g0 = tile * GROUPS + wave * (GROUPS / 4);
    const _Float16 *in = act1 + (size_t)clip * T * H1 * W1 * C1;
    int pt[MT], py[MT], px[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int g = g0 + mt * 4 + (r >> 3), e = r & 7;
        pv[mt] = g < NG;
        const int gg = pv[mt] ? g : 0;
        pt[mt] = 2 * (gg / (H2 * W2)) + (e >> 2);
        py[mt] = 2 * ((gg / W2) % H2) + ((e >> 1) & 1);
        px[mt] = 2 * (gg % W2) + (e & 1);
    }
    f32x16 acc[MT][NT] = {};
    if constexpr (WLDS) f16_conv_taps_wlds<C1, 3>(acc, in, w2, pt, py, px, pv, T, H1, W1);
    else f16_conv_taps<C1, 3>(acc, in, w2, pt, py, px, pv, T, H1, W1);
    _Float16 *out = act2 + (size_t)clip * NG * C2;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = nt * 32 + r;
        const float bias = b2[co];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = fmaxf(fmaxf(acc[mt][nt][4 * j], acc[mt][nt][4 * j + 1]), fmaxf(acc[mt][nt][4 * j + 2], acc[mt][nt][4 * j + 3]));
                v = fmaxf(v, __shfl_xor(v, 32));
                const int g = g0 + mt * 4 + j;
                if ((j & 1) == h && g < NG) out[(size_t)g * C2 + co] = (_Float16)fmaxf(v + bias, 0.f);
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// K_conv3.  Block = 256 positions (linear over [T2][H2][W2]; four waves of 64) of one clip x 128 of the 256 channels
// (blockIdx.y = channel half).  Epilogue: f32_tile_sum (bias + ReLU, then the tile's per-channel sum), fp32.
template <bool WLDS>
__global__ void __launch_bounds__(256) k_c3d16_conv3(const _Float16 *act2, const _Float16 *w3, const float *b3, float *partial, int T2,
                                                     int H2, int W2, int tiles)
{
    const int clip = blockIdx.z, cb = blockIdx.y, tile = blockIdx.x;
    const int r = threadIdx.x & 31, wave = threadIdx.x >> 6;
    const int P = T2 * H2 * W2;
    const int m0 = tile * 256 + wave * 64;
    int pt[MT], py[MT], px[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int p = m0 + mt * 32 + r;
        pv[mt] = p < P;
        const int pp = pv[mt] ? p : 0;
        pt[mt] = pp / (H2 * W2);
        py[mt] = (pp / W2) % H2;
        px[mt] = pp % W2;
    }
    f32x16 acc[MT][NT] = {};
    if constexpr (WLDS) f16_conv_taps_wlds<C2, 3>(acc, act2 + (size_t)clip * P * C2, w3 + (size_t)cb * C2 * TAPS * C2, pt, py, px, pv, T2, H2, W2);
    else f16_conv_taps<C2, 3>(acc, act2 + (size_t)clip * P * C2, w3 + (size_t)cb * C2 * TAPS * C2, pt, py, px, pv, T2, H2, W2);
    f32_tile_sum(acc, b3 + cb * C2, m0, P, partial + ((size_t)clip * tiles + tile) * C3 + cb * C2);
}

// `n` fp32 values rounded once to fp16 (round to nearest even); false if one does not stay finite
bool round_f16(const float *src, size_t n, std::vector<_Float16> &dst)
{
    dst.resize(n);
    for (size_t i = 0; i < n; ++i) {
        dst[i] = (_Float16)src[i];
        if (!std::isfinite((float)dst[i])) return false;
    }
    return true;
}

}  // namespace

struct rva_cnn3d_f16_plan {
    rva_ctx *ctx = nullptr;
    rva_cnn3d_desc d{};
    int H1 = 0, W1 = 0, T2 = 0, H2 = 0, W2 = 0, conv1_tiles_x = 0, conv1_tiles = 0, conv2_tiles = 0, conv3_tiles = 0;
    float *w1 = nullptr, *b1 = nullptr, *b2 = nullptr, *b3 = nullptr, *wh = nullptr, *bh = nullptr;
    _Float16 *w2 = nullptr, *w3 = nullptr, *act1 = nullptr, *act2 = nullptr;
    float *partial = nullptr, *feat = nullptr;
    int wlds = 3;                                    // bit 0 / 1: conv2 / conv3 stage their weights through LDS (A/B switch RVA_C3D16_WLDS)
    rva_dev_arena mem;

    // the arena hands out floats: n fp16 elements take (n + 1) / 2 of them
    int alloc_h(_Float16 **dst, size_t n) { return mem.alloc(ctx, reinterpret_cast<float **>(dst), (n + 1) / 2); }
    int upload_h(_Float16 **dst, const std::vector<_Float16> &src)
    {
        const int rc = alloc_h(dst, src.size());
        if (rc != RVA_OK) return rc;
        RVA_HIP(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        return RVA_OK;
    }
};

extern "C" {

int rva_cnn3d_f16_plan_create(rva_ctx *ctx, const rva_cnn3d_desc *desc, const rva_cnn3d_weights *wt, rva_cnn3d_f16_plan **out)
{
    if (!ctx || !desc || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_f16_plan_create: null argument");
    *out = nullptr;
    const rva_cnn3d_desc d = *desc;
    // the pools floor: (1,2,2) then (2,2,2) leave nothing of fewer than 2 frames or 4 rows / columns (torch fails there too)
    if (d.height < 4 || d.width < 4 || d.frames < 2 || d.classes < 1 || d.classes > MAX_CLASSES || d.max_clips < 1 ||
        (int64_t)d.max_clips * d.frames > 65535 || (int64_t)d.height * d.width > (1 << 26))
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_f16_plan_create: bad descriptor (height, width >= 4, frames >= 2, classes 1..%d, "
                        "max_clips >= 1, max_clips * frames <= 65535)", MAX_CLASSES);
    if (!wt->conv1_w || !wt->conv1_b || !wt->conv2_w || !wt->conv2_b || !wt->conv3_w || !wt->conv3_b || !wt->head_w || !wt->head_b)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_f16_plan_create: every weight array is required");
    const size_t n_w1 = (size_t)C1 * 3 * TAPS, n_w2 = (size_t)C2 * TAPS * C1, n_w3 = (size_t)C3 * TAPS * C2;
    std::vector<_Float16> h1, h2, h3;
    const char *bad = !round_f16(wt->conv1_w, n_w1, h1) ? "conv1_w" : !round_f16(wt->conv2_w, n_w2, h2) ? "conv2_w" :
                      !round_f16(wt->conv3_w, n_w3, h3) ? "conv3_w" : nullptr;
    if (bad) return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_f16_plan_create: a value of %s does not stay finite in fp16", bad);
    std::vector<float> w1f(n_w1);                       // K_conv1 keeps its weights in fp32 registers: the fp16 values, widened
    for (size_t i = 0; i < n_w1; ++i) w1f[i] = (float)h1[i];
    auto *p = new rva_cnn3d_f16_plan();
    p->ctx = ctx;
    p->d = d;
    if (const char *e = getenv("RVA_C3D16_WLDS")) p->wlds = atoi(e);
    const int T = d.frames;
    p->H1 = d.height / 2; p->W1 = d.width / 2;
    p->T2 = T / 2; p->H2 = p->H1 / 2; p->W2 = p->W1 / 2;
    const size_t ng = (size_t)p->T2 * p->H2 * p->W2;
    p->conv1_tiles_x = rva_ceil_div(p->W1, PT);
    p->conv1_tiles = p->conv1_tiles_x * rva_ceil_div(p->H1, PT);
    p->conv2_tiles = (int)((ng + GROUPS - 1) / GROUPS);
    p->conv3_tiles = (int)((ng + 255) / 256);
    const size_t mc = (size_t)d.max_clips;
    const size_t n_act1 = mc * T * p->H1 * p->W1 * C1, n_act2 = mc * ng * C2, n_part = mc * p->conv3_tiles * C3, n_feat = mc * C3;
    const size_t need = (n_act1 + n_act2 + n_w2 + n_w3) * sizeof(_Float16) +
                        (n_part + n_feat + n_w1 + C1 + C2 + C3 + (size_t)d.classes * (C3 + 1)) * sizeof(float);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b) {
        delete p;
        return rva_fail(ctx, RVA_ERR_CAPACITY, "rva_cnn3d_f16_plan_create: the workspace for %d clips of %d x %d x %d needs %zu MB, the "
                        "device has %zu MB free", d.max_clips, T, d.height, d.width, need >> 20, free_b >> 20);
    }
    int rc = RVA_OK;
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    step(p->mem.upload(ctx, &p->w1, w1f.data(), n_w1));
    step(p->mem.upload(ctx, &p->b1, wt->conv1_b, C1));
    step(p->upload_h(&p->w2, h2));
    step(p->mem.upload(ctx, &p->b2, wt->conv2_b, C2));
    step(p->upload_h(&p->w3, h3));
    step(p->mem.upload(ctx, &p->b3, wt->conv3_b, C3));
    step(p->mem.upload(ctx, &p->wh, wt->head_w, (size_t)d.classes * C3));
    step(p->mem.upload(ctx, &p->bh, wt->head_b, d.classes));
    step(p->alloc_h(&p->act1, n_act1));
    step(p->alloc_h(&p->act2, n_act2));
    step(p->mem.alloc(ctx, &p->partial, n_part));
    step(p->mem.alloc(ctx, &p->feat, n_feat));
    if (rc == RVA_OK) rc = rva_clip_head_prepare(ctx, C3);
    if (rc == RVA_OK) rc = rva_clip_post_prepare(ctx, d.classes);
    if (rc != RVA_OK) {
        rva_cnn3d_f16_plan_destroy(p);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

void rva_cnn3d_f16_plan_destroy(rva_cnn3d_f16_plan *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

int rva_cnn3d_f16_plan_info(const rva_cnn3d_f16_plan *p, int32_t *pool1, int32_t *pool2, int32_t *tiles, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    if (pool1) { pool1[0] = p->d.frames; pool1[1] = p->H1; pool1[2] = p->W1; }
    if (pool2) { pool2[0] = p->T2; pool2[1] = p->H2; pool2[2] = p->W2; }
    if (tiles) { tiles[0] = p->conv1_tiles; tiles[1] = p->conv2_tiles; tiles[2] = p->conv3_tiles; }
    if (n_launches) *n_launches = 5;
    return RVA_OK;
}

int rva_cnn3d_f16_plan_run(rva_cnn3d_f16_plan *p, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                           rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_f16_plan_run: bad argument (n_clips %d, capacity %d)", n_clips, p->d.max_clips);
    const hipStream_t st = (hipStream_t)stream_;
    const int T = p->d.frames;
    k_c3d16_conv1<<<dim3(p->conv1_tiles, n_clips * T), CONV1_THREADS, 0, st>>>((const _Float16 *)frames, frame_index, p->w1, p->b1,
                                                                               p->act1, T, p->d.height, p->d.width, p->H1, p->W1,
                                                                               p->conv1_tiles_x);
    RVA_HIP(ctx, hipGetLastError());
    if (p->wlds & 1)
        k_c3d16_conv2<true><<<dim3(p->conv2_tiles, n_clips), 256, 0, st>>>(p->act1, p->w2, p->b2, p->act2, T, p->H1, p->W1, p->T2, p->H2, p->W2);
    else
        k_c3d16_conv2<false><<<dim3(p->conv2_tiles, n_clips), 256, 0, st>>>(p->act1, p->w2, p->b2, p->act2, T, p->H1, p->W1, p->T2, p->H2, p->W2);
    RVA_HIP(ctx, hipGetLastError());
    if (p->wlds & 2)
        k_c3d16_conv3<true><<<dim3(p->conv3_tiles, 2, n_clips), 256, 0, st>>>(p->act2, p->w3, p->b3, p->partial, p->T2, p->H2, p->W2, p->conv3_tiles);
    else
        k_c3d16_conv3<false><<<dim3(p->conv3_tiles, 2, n_clips), 256, 0, st>>>(p->act2, p->w3, p->b3, p->partial, p->T2, p->H2, p->W2, p->conv3_tiles);
    RVA_HIP(ctx, hipGetLastError());
    int rc = rva_clip_mean_launch(ctx, p->partial, p->conv3_tiles, (float)((size_t)p->T2 * p->H2 * p->W2), p->feat, n_clips, C3, st);
    if (rc != RVA_OK) return rc;
    return rva_clip_head_launch(ctx, p->feat, p->wh, p->bh, (float *)logits, C3, p->d.classes, n_clips, st);
}

int rva_cnn3d_f16_plan_run_post(rva_cnn3d_f16_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                                void *cls, void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, "rva_cnn3d_f16_plan_run_post", (const float *)logits, p->d.classes, std::min(5, p->d.classes), rows, n_rows,
                                max_det, (float *)scores, (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  Every tensor is clip-major; ACT1 / ACT2
// are fp16 elements, PARTIAL / FEAT fp32, and the counts are element counts.
int rva_cnn3d_f16_plan_stage(rva_cnn3d_f16_plan *p, int stage, int n_clips, void *dst, int64_t dst_elems, int64_t *n_elems,
                             rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_f16_plan_stage: bad argument (n_clips %d, capacity %d)", n_clips, p->d.max_clips);
    const int64_t ng = (int64_t)p->T2 * p->H2 * p->W2;
    const void *src = nullptr;
    int64_t count = 0;
    size_t esize = sizeof(float);
    switch (stage) {
    case RVA_CNN3D_STAGE_ACT1: src = p->act1; count = (int64_t)n_clips * p->d.frames * p->H1 * p->W1 * C1; esize = sizeof(_Float16); break;
    case RVA_CNN3D_STAGE_ACT2: src = p->act2; count = (int64_t)n_clips * ng * C2; esize = sizeof(_Float16); break;
    case RVA_CNN3D_STAGE_PARTIAL: src = p->partial; count = (int64_t)n_clips * p->conv3_tiles * C3; break;
    case RVA_CNN3D_STAGE_FEAT: src = p->feat; count = (int64_t)n_clips * C3; break;
    default: return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_f16_plan_stage: unknown stage %d", stage);
    }
    if (n_elems) *n_elems = count;
    if (!dst) return RVA_OK;
    if (dst_elems < count)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_f16_plan_stage: dst holds %lld elements, stage %d of %d clips has %lld",
                        (long long)dst_elems, stage, n_clips, (long long)count);
    RVA_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)count * esize, hipMemcpyDeviceToDevice, (hipStream_t)stream_));
    return RVA_OK;
}

}  // extern "C"
