// fp32 3D-CNN clip network (the reference's 3D-CNN head, scripts/convert_temporal_model_to_onnx.py:91-121) as one plan object:
//
//   per clip [3,T,H,W]: Conv3d(3,64,3,p1)+BN+ReLU -> MaxPool3d((1,2,2)) -> Conv3d(64,128,3,p1)+BN+ReLU -> MaxPool3d(2)
//                       -> Conv3d(128,256,3,p1)+BN+ReLU -> mean over T,H,W -> Linear(256 -> classes) -> top-k (k = min(5, classes))
//
// Everything is fp32 (BatchNorm is folded by the caller in float64 and rounded once); activations are channels-last
// ([T][H][W][C]).  The contracts are those of rva_clip.hip: every sum runs in ONE fixed order that depends neither on the number
// of clips, nor on a clip's position in the batch, nor on the launch mode -- no split-K whose order follows the grid and no
// float atomics -- so logits are bit-identical across batch sizes, clip positions, an index-table permutation of the ring,
// eager launches and hipGraph replay.  The pools follow torch (floor, no padding): trailing odd rows, columns and frames are
// dropped and the convolution outputs that only feed them are not computed.  A max commutes exactly with the monotonic
// "+ bias, ReLU", so the pools take the max of the raw sums first.  The launches of one pass (rva_cnn3d_plan_run):
//
//   K_conv1  conv1 + 2x2 spatial max pool + bias + ReLU, 8x8 pooled tile of one frame per block; reads the planar frames straight
//            from the caller's ring through the device table of frame indices (frame t of clip b and its temporal neighbours
//            are entries b*T + t - 1 .. b*T + t + 1; zero outside the clip).  VALU fmaf, taps in the checkpoint's (ci, kt, ky,
//            kx) order.  Writes [T][H/2][W/2][64].
//   K_conv2  27 taps x 64 channels on the exact fp32-input MFMA core of rva_mfma_f32.h (which defines the reduction order); a block owns 32 whole 2x2x2 pool
//            groups, so the max pool + bias + ReLU run in the epilogue and the unpooled 128-channel volume is never written.
//            Writes [T/2][H/4][W/4][128].
//   K_conv3  27 taps x 128 channels, same core; bias + ReLU, then the tile's per-channel sum (positions in tile order): the
//            256-channel volume is never written.
//   K_mean   a clip's tile partials reduced in tile order and divided by T'*H'*W': the mean kernel of rva_clip.hip.
//   K_head   Linear: the head kernel of rva_clip.hip (one thread per class, k in order).
//   K_post   (rva_cnn3d_plan_run_post) the top-k kernel of rva_clip.hip.
#include "rva_internal.h"
#include "rva_mfma_f32.h"

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
// K_conv1.  Thread = output channel (tid & 63) x a wave-uniform pooled position, so the input reads are LDS broadcasts and each
// thread keeps its 81 weights in registers.  The four conv outputs under a pooled position share one 4x4 input window per
// (channel, frame).  Sum of a conv output: fmaf chain from 0 over (ci, kt, ky, kx) in order; then max of the four, + bias, ReLU.
__global__ void __launch_bounds__(CONV1_THREADS) k_c3d_conv1(const float *ring, const int32_t *frame_index, const float *w1,
                                                             const float *b1, float *act1, int T, int H, int W, int H1, int W1,
                                                             int tiles_x)
{
    __shared__ float xin[3 * 3 * IT * ITW];                // [kt][ci][IT][ITW]
    const int f = blockIdx.y, t = f % T;
    const int py0 = (blockIdx.x / tiles_x) * PT, px0 = (blockIdx.x % tiles_x) * PT;
    const int iy0 = 2 * py0 - 1, ix0 = 2 * px0 - 1;
    for (int kt = 0; kt < 3; ++kt) {
        const int tt = t + kt - 1;
        const bool tv = (unsigned)tt < (unsigned)T;       // block-uniform
        const float *img = tv ? ring + (size_t)frame_index[f + kt - 1] * 3 * H * W : ring;
        for (int i = threadIdx.x; i < 3 * IT * IT; i += CONV1_THREADS) {
            const int c = i / (IT * IT), rr = (i / IT) % IT, q = i % IT;
            const int iy = iy0 + rr, ix = ix0 + q;
            xin[((kt * 3 + c) * IT + rr) * ITW + q] =
                (tv && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) ? img[((size_t)c * H + iy) * W + ix] : 0.f;
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
        act1[(((size_t)f * H1 + py) * W1 + px) * C1 + co] = fmaxf(m + bias, 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------
// K_conv2.  Block = 32 pool groups (linear over [T2][H2][W2]) of one clip x all 128 channels; wave = 8 groups = 64 conv positions.
// Row m of a wave's 64: group m >> 3, position (dt, dy, dx) = bits 2, 1, 0 of m & 7 inside it.  C/D map (f32_cd_row): column =
// lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) -- so registers 4j .. 4j+3 of a lane are half a pool group and the other
// lane half holds the rest.  Epilogue: max of the eight raw sums, + bias, ReLU.
__global__ void __launch_bounds__(256) k_c3d_conv2(const float *act1, const float *w2, const float *b2, float *act2, int T, int H1,
                                                   int W1, int T2, int H2, int W2)
{
    const int clip = blockIdx.y, tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int NG = T2 * H2 * W2;
    const int g0 = tile * GROUPS + wave * (GROUPS / 4);
    const float *in = act1 + (size_t)clip * T * H1 * W1 * C1;
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
    f32_conv_taps<C1, 3>(acc, in, w2, pt, py, px, pv, T, H1, W1);
    float *out = act2 + (size_t)clip * NG * C2;
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
                if ((j & 1) == h && g < NG) out[(size_t)g * C2 + co] = fmaxf(v + bias, 0.f);
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// K_conv3.  Block = 256 positions (linear over [T2][H2][W2]; four waves of 64) of one clip x 128 of the 256 channels
// (blockIdx.y = channel half).  Epilogue: f32_tile_sum (bias + ReLU, then the tile's per-channel sum).
__global__ void __launch_bounds__(256) k_c3d_conv3(const float *act2, const float *w3, const float *b3, float *partial, int T2, int H2,
                                                   int W2, int tiles)
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
    f32_conv_taps<C2, 3>(acc, act2 + (size_t)clip * P * C2, w3 + (size_t)cb * C2 * TAPS * C2, pt, py, px, pv, T2, H2, W2);
    f32_tile_sum(acc, b3 + cb * C2, m0, P, partial + ((size_t)clip * tiles + tile) * C3 + cb * C2);
}

}  // namespace

struct rva_cnn3d_plan {
    rva_ctx *ctx = nullptr;
    rva_cnn3d_desc d{};
    int H1 = 0, W1 = 0, T2 = 0, H2 = 0, W2 = 0, conv1_tiles_x = 0, conv1_tiles = 0, conv2_tiles = 0, conv3_tiles = 0;
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr, *wh = nullptr, *bh = nullptr;
    float *act1 = nullptr, *act2 = nullptr, *partial = nullptr, *feat = nullptr;
    rva_dev_arena mem;
};

extern "C" {

int rva_cnn3d_plan_create(rva_ctx *ctx, const rva_cnn3d_desc *desc, const rva_cnn3d_weights *wt, rva_cnn3d_plan **out)
{
    if (!ctx || !desc || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_plan_create: null argument");
    *out = nullptr;
    const rva_cnn3d_desc d = *desc;
    // the pools floor: (1,2,2) then (2,2,2) leave nothing of fewer than 2 frames or 4 rows / columns (torch fails there too)
    if (d.height < 4 || d.width < 4 || d.frames < 2 || d.classes < 1 || d.classes > MAX_CLASSES || d.max_clips < 1 ||
        (int64_t)d.max_clips * d.frames > 65535 || (int64_t)d.height * d.width > (1 << 26))
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_plan_create: bad descriptor (height, width >= 4, frames >= 2, classes 1..%d, "
                        "max_clips >= 1, max_clips * frames <= 65535)", MAX_CLASSES);
    if (!wt->conv1_w || !wt->conv1_b || !wt->conv2_w || !wt->conv2_b || !wt->conv3_w || !wt->conv3_b || !wt->head_w || !wt->head_b)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_plan_create: every weight array is required");
    auto *p = new rva_cnn3d_plan();
    p->ctx = ctx;
    p->d = d;
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
    const size_t n_w = (size_t)C1 * 3 * TAPS + C1 + (size_t)C2 * TAPS * C1 + C2 + (size_t)C3 * TAPS * C2 + C3 + (size_t)d.classes * (C3 + 1);
    const size_t need = (n_act1 + n_act2 + n_part + n_feat + n_w) * sizeof(float);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b) {
        delete p;
        return rva_fail(ctx, RVA_ERR_CAPACITY, "rva_cnn3d_plan_create: the workspace for %d clips of %d x %d x %d needs %zu MB, the "
                        "device has %zu MB free", d.max_clips, T, d.height, d.width, need >> 20, free_b >> 20);
    }
    int rc = RVA_OK;
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    step(p->mem.upload(ctx, &p->w1, wt->conv1_w, (size_t)C1 * 3 * TAPS));
    step(p->mem.upload(ctx, &p->b1, wt->conv1_b, C1));
    step(p->mem.upload(ctx, &p->w2, wt->conv2_w, (size_t)C2 * TAPS * C1));
    step(p->mem.upload(ctx, &p->b2, wt->conv2_b, C2));
    step(p->mem.upload(ctx, &p->w3, wt->conv3_w, (size_t)C3 * TAPS * C2));
    step(p->mem.upload(ctx, &p->b3, wt->conv3_b, C3));
    step(p->mem.upload(ctx, &p->wh, wt->head_w, (size_t)d.classes * C3));
    step(p->mem.upload(ctx, &p->bh, wt->head_b, d.classes));
    step(p->mem.alloc(ctx, &p->act1, n_act1));
    step(p->mem.alloc(ctx, &p->act2, n_act2));
    step(p->mem.alloc(ctx, &p->partial, n_part));
    step(p->mem.alloc(ctx, &p->feat, n_feat));
    if (rc == RVA_OK) rc = rva_clip_head_prepare(ctx, C3);
    if (rc == RVA_OK) rc = rva_clip_post_prepare(ctx, d.classes);
    if (rc != RVA_OK) {
        rva_cnn3d_plan_destroy(p);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

void rva_cnn3d_plan_destroy(rva_cnn3d_plan *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

int rva_cnn3d_plan_info(const rva_cnn3d_plan *p, int32_t *pool1, int32_t *pool2, int32_t *tiles, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    if (pool1) { pool1[0] = p->d.frames; pool1[1] = p->H1; pool1[2] = p->W1; }
    if (pool2) { pool2[0] = p->T2; pool2[1] = p->H2; pool2[2] = p->W2; }
    if (tiles) { tiles[0] = p->conv1_tiles; tiles[1] = p->conv2_tiles; tiles[2] = p->conv3_tiles; }
    if (n_launches) *n_launches = 5;
    return RVA_OK;
}

int rva_cnn3d_plan_run(rva_cnn3d_plan *p, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                       rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_plan_run: bad argument (n_clips %d, capacity %d)", n_clips, p->d.max_clips);
    const hipStream_t st = (hipStream_t)stream_;
    const int T = p->d.frames;
    k_c3d_conv1<<<dim3(p->conv1_tiles, n_clips * T), CONV1_THREADS, 0, st>>>((const float *)frames, frame_index, p->w1, p->b1, p->act1,
                                                                             T, p->d.height, p->d.width, p->H1, p->W1, p->conv1_tiles_x);
    RVA_HIP(ctx, hipGetLastError());
    k_c3d_conv2<<<dim3(p->conv2_tiles, n_clips), 256, 0, st>>>(p->act1, p->w2, p->b2, p->act2, T, p->H1, p->W1, p->T2, p->H2, p->W2);
    RVA_HIP(ctx, hipGetLastError());
    k_c3d_conv3<<<dim3(p->conv3_tiles, 2, n_clips), 256, 0, st>>>(p->act2, p->w3, p->b3, p->partial, p->T2, p->H2, p->W2, p->conv3_tiles);
    RVA_HIP(ctx, hipGetLastError());
    int rc = rva_clip_mean_launch(ctx, p->partial, p->conv3_tiles, (float)((size_t)p->T2 * p->H2 * p->W2), p->feat, n_clips, C3, st);
    if (rc != RVA_OK) return rc;
    return rva_clip_head_launch(ctx, p->feat, p->wh, p->bh, (float *)logits, C3, p->d.classes, n_clips, st);
}

int rva_cnn3d_plan_run_post(rva_cnn3d_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                            void *cls, void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, "rva_cnn3d_plan_run_post", (const float *)logits, p->d.classes, std::min(5, p->d.classes), rows, n_rows, max_det,
                                (float *)scores, (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  Every tensor is clip-major.
int rva_cnn3d_plan_stage(rva_cnn3d_plan *p, int stage, int n_clips, void *dst, int64_t dst_floats, int64_t *n_floats,
                         rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_plan_stage: bad argument (n_clips %d, capacity %d)", n_clips, p->d.max_clips);
    const int64_t ng = (int64_t)p->T2 * p->H2 * p->W2;
    const float *src = nullptr;
    int64_t count = 0;
    switch (stage) {
    case RVA_CNN3D_STAGE_ACT1: src = p->act1; count = (int64_t)n_clips * p->d.frames * p->H1 * p->W1 * C1; break;
    case RVA_CNN3D_STAGE_ACT2: src = p->act2; count = (int64_t)n_clips * ng * C2; break;
    case RVA_CNN3D_STAGE_PARTIAL: src = p->partial; count = (int64_t)n_clips * p->conv3_tiles * C3; break;
    case RVA_CNN3D_STAGE_FEAT: src = p->feat; count = (int64_t)n_clips * C3; break;
    default: return rva_fail(ctx, RVA_ERR_ARG, "rva_cnn3d_plan_stage: unknown stage %d", stage);
    }
    return rva_clip_stage_copy(ctx, "rva_cnn3d_plan_stage", stage, n_clips, src, count, 0, 0, 0, dst, dst_floats, n_floats,
                               (hipStream_t)stream_);
}

}  // extern "C"
