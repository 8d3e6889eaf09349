// fp32 CNN-LSTM clip network (the reference's temporal head, scripts/convert_temporal_model_to_onnx.py:34-88) as one plan object:
//
//   per frame: Conv2d(3,64,7,s2,p3)+BN+ReLU -> MaxPool(3,s2,p1) -> Conv2d(64,128,3,p1)+BN+ReLU -> mean over H,W
//   per clip:  LSTM(128 -> hidden, 2 layers, gates i,f,g,o) -> Linear(hidden -> classes) on h2[T-1] -> top-k (k = min(5, classes))
//
// Everything is fp32 (BatchNorm is folded by the caller in float64 and rounded once).  Every sum runs in ONE fixed order that
// depends neither on the batch (number of clips), nor on a clip's position in it, nor on the launch mode: no split-K whose
// order follows the grid and no float atomics.  Logits are therefore bit-identical across batch sizes, clip positions, eager
// launches and hipGraph replay.  The launches of one pass (rva_cnnlstm_plan_run):
//
//   K_stem   conv1 + bias + ReLU + 3x3/s2 max pool, 8x8 pooled tile per block (17x17 conv tile incl. the pool halo in LDS);
//            reads the planar frames straight from the caller's ring through a device table of frame indices.  VALU fmaf,
//            taps in the checkpoint's (ci, ky, kx) order.  NHWC out.
//   K_conv2  3x3 conv on the exact fp32-input MFMA core of rva_mfma_f32.h (which defines the reduction order), bias + ReLU, then
//            the tile's per-channel sum (pixels in tile order): the 128-channel map itself is never written.
//   K_mean   partial sums of a frame reduced in tile order and divided by H*W: the spatial mean, once per frame.
//   K_xproj  layer 1's input projection X.W_ih1^T + (b_ih1 + b_hh1) for all T steps.
//   K_lstm   T+1 "diagonal" launches: launch s runs layer 1 at step s and layer 2 at step s-1 (both read h1[s-1]).  A block owns
//            four hidden units and all four gates of them for every clip; consecutive launches order the steps (no grid barrier).
//   K_head   Linear on h2[T-1]: one thread per class, k in order.
//   K_post   (rva_cnnlstm_plan_run_post) top-k per result row by rank counting, boxes (0, 0, w, h), counts; rows without a clip
//            get count 0.
#include "rva_clip_host.h"
#include "rva_lstm_dev.h"

namespace {

constexpr int C1 = CL_C1, C2 = CL_C2, K1 = CL_K1;         // stem widths of the architecture
constexpr int PT = CL_PT;                                  // pooled tile (PT x PT) of K_stem
constexpr int CT = 2 * PT + 1;                             // conv rows of that tile, pool halo included (17)
constexpr int CTW = CT + 1;                                // conv columns (18: pairs of adjacent outputs per thread)
constexpr int IT = 2 * (CT - 1) + K1;                      // input rows of the tile (39)
constexpr int ITW = 2 * (CTW - 1) + K1 + 1;                // input columns, padded (42)
constexpr int STEM_THREADS = 512;
constexpr size_t STEM_LDS = (size_t)(CT * CTW * C1 + 3 * IT * ITW) * sizeof(float);

// ---------------------------------------------------------------------------------------------------
// K_stem.  Thread = output channel (tid & 63) x a wave-uniform conv position pair, so the input reads are LDS broadcasts and
// each thread keeps its 147 weights in registers.  Conv positions outside the conv map hold -inf (the pool's padding); after
// ReLU every real value is >= 0.
__global__ void __launch_bounds__(STEM_THREADS) k_clip_stem(const float *ring, const int32_t *frame_index, const float *w1,
                                                           const float *b1, float *pooled, int H, int W, int Hc, int Wc, int Hp,
                                                           int Wp, int tiles_x)
{
    extern __shared__ float lds[];
    float *conv = lds;                                     // [CT][CTW][C1]
    float *xin = lds + CT * CTW * C1;                      // [3][IT][ITW]
    const int f = blockIdx.y;
    const int py0 = (blockIdx.x / tiles_x) * PT, px0 = (blockIdx.x % tiles_x) * PT;
    const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;        // first conv row / column of the tile
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;        // first input row / column
    const float *img = ring + (size_t)frame_index[f] * 3 * H * W;
    for (int i = threadIdx.x; i < 3 * IT * ITW; i += STEM_THREADS) {
        const int c = i / (IT * ITW), r = (i / ITW) % IT, q = i % ITW;
        const int iy = iy0 + r, ix = ix0 + q;
        xin[i] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) ? img[((size_t)c * H + iy) * W + ix] : 0.f;
    }
    const int co = threadIdx.x & (C1 - 1), grp = threadIdx.x >> 6;
    float w[3 * K1 * K1];
#pragma unroll
    for (int t = 0; t < 3 * K1 * K1; ++t) w[t] = w1[co * 3 * K1 * K1 + t];
    const float bias = b1[co];
    __syncthreads();
    constexpr int NPAIR = CT * (CTW / 2);
    for (int pr = grp; pr < NPAIR; pr += STEM_THREADS / 64) {
        const int ly = pr / (CTW / 2), lx = 2 * (pr % (CTW / 2));
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int ky = 0; ky < K1; ++ky) {
                const float *xr = xin + (c * IT + 2 * ly + ky) * ITW + 2 * lx;
                float x[K1 + 2];
#pragma unroll
                for (int j = 0; j < K1 + 2; ++j) x[j] = xr[j];
#pragma unroll
                for (int kx = 0; kx < K1; ++kx) {
                    const float wv = w[(c * K1 + ky) * K1 + kx];
                    s0 = fmaf(x[kx], wv, s0);
                    s1 = fmaf(x[kx + 2], wv, s1);
                }
            }
        const int cy = cy0 + ly, cx = cx0 + lx;
        const bool vy = (unsigned)cy < (unsigned)Hc;
        conv[(ly * CTW + lx) * C1 + co] = vy && (unsigned)cx < (unsigned)Wc ? fmaxf(s0 + bias, 0.f) : -INFINITY;
        conv[(ly * CTW + lx + 1) * C1 + co] = vy && (unsigned)(cx + 1) < (unsigned)Wc ? fmaxf(s1 + bias, 0.f) : -INFINITY;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PT * PT * C1; i += STEM_THREADS) {
        const int c = i & (C1 - 1), p = i >> 6;
        const int ly = p / PT, lx = p % PT, py = py0 + ly, px = px0 + lx;
        if (py >= Hp || px >= Wp) continue;
        float m = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, conv[((2 * ly + dy) * CTW + 2 * lx + dx) * C1 + c]);
        pooled[(((size_t)f * Hp + py) * Wp + px) * C1 + c] = m;
    }
}

// ---------------------------------------------------------------------------------------------------
// K_conv2.  NHWC implicit GEMM, one frame per grid row: block = 256 pixels of the frame (four waves of 64) x all 128 channels.
// Reduction order and epilogue (bias + ReLU, then the tile's per-channel sum) are rva_mfma_f32.h's: 9 taps x two chunks of 32
// channels -- what rva_conv2d_nhwc_f32_v runs on the same input -- then f32_tile_sum.
__global__ void __launch_bounds__(256) k_clip_conv2(const float *pooled, const float *w2, const float *b2, float *partial, int Hp,
                                                    int Wp, int tiles)
{
    constexpr int MT = 2, NT = 4;
    const int f = blockIdx.y, tile = blockIdx.x;
    const int r = threadIdx.x & 31, wave = threadIdx.x >> 6;
    const int P = Hp * Wp;
    const int m0 = tile * 256 + wave * 64;
    int pt[MT], py[MT], px[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int p = m0 + mt * 32 + r;
        pv[mt] = p < P;
        pt[mt] = 0;
        py[mt] = pv[mt] ? p / Wp : 0;
        px[mt] = pv[mt] ? p % Wp : 0;
    }
    f32x16 acc[MT][NT] = {};
    f32_conv_taps<C1, 1>(acc, pooled + (size_t)f * P * C1, w2, pt, py, px, pv, 1, Hp, Wp);
    f32_tile_sum(acc, b2, m0, P, partial + ((size_t)f * tiles + tile) * C2);
}

// ---------------------------------------------------------------------------------------------------
// K_mean.  Block = row (a frame here, a clip in rva_clip3d.hip), thread = channel, blockDim.x channels: feat[row][c] = (sum of
// the row's tile partials in tile order) / n.
__global__ void __launch_bounds__(256) k_clip_mean(const float *partial, int tiles, float n, float *feat)
{
    const int row = blockIdx.x, c = threadIdx.x, C = blockDim.x;
    const float *pp = partial + (size_t)row * tiles * C + c;
    float s = 0.f;
    for (int k = 0; k < tiles; ++k) s = s + pp[(size_t)k * C];
    feat[(size_t)row * C + c] = s / n;
}

// ---------------------------------------------------------------------------------------------------
// K_xproj: clip_xproj (rva_lstm_dev.h) with W_ih1 fp32.
__global__ void __launch_bounds__(256) k_clip_xproj(const float *feat_g, const float *wih1, const float *b1, float *gx, int T, int G4)
{
    clip_xproj(feat_g, wih1, b1, gx, T, G4);
}

// ---------------------------------------------------------------------------------------------------
// K_lstm, launch s: clip_lstm (rva_lstm_dev.h) with W_hh1 and [W_ih2 | W_hh2] fp32, row-major.
__global__ void __launch_bounds__(256) k_clip_lstm(int s, int T, int hidden, int n_clips, int cap, const float *whh1, const float *w2,
                                                   const float *gx, const float *b2, float *h1, float *h2, float *c1, float *c2)
{
    clip_lstm(s, T, hidden, n_clips, cap, whh1, w2, gx, b2, h1, h2, c1, c2);
}

// ---------------------------------------------------------------------------------------------------
// K_head: logits[clip][n] = (sum_k W[n][k] * h2[T-1][clip][k], k in order) + bias[n]
__global__ void __launch_bounds__(256) k_clip_head(const float *hlast, const float *wh, const float *bh, float *logits, int hidden,
                                                   int classes)
{
    extern __shared__ float hv[];
    const int clip = blockIdx.y;
    for (int k = threadIdx.x; k < hidden; k += 256) hv[k] = hlast[(size_t)clip * hidden + k];
    __syncthreads();
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= classes) return;
    const float *wr = wh + (size_t)n * hidden;
    float s = 0.f;
    for (int k = 0; k < hidden; ++k) s = fmaf(wr[k], hv[k], s);
    logits[(size_t)clip * classes + n] = s + bh[n];
}

// ---------------------------------------------------------------------------------------------------
// K_post: block = result row.  rows[3 * row] = clip of the row or -1, rows[3 * row + 1 .. 2] = (w, h) of the clip's frames.
// The top k by the reference rule (ascending stable sort, last k reversed, temporal_detector.py:396-398) in torch.sort's order
// (the rule of stage_post): class n ranks at #{m : above(m, n)}, where m is above n if v[m] > v[n], or v[m] == v[n] and m > n
// (exact ties put the larger class index first); NaN counts as larger than every number (NaN against NaN: the index decides).
__device__ inline bool clip_above(float a, int m, float b, int n)
{
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || m > n);
    return a > b || (a == b && m > n);
}

__global__ void __launch_bounds__(256) k_clip_post(const float *logits, int classes, const int32_t *rows, int k, int max_det,
                                                   float *scores, int32_t *cls, float *boxes, int32_t *counts)
{
    extern __shared__ float v[];
    const int row = blockIdx.x;
    const int clip = rows[3 * row];
    if (clip < 0) {
        if (threadIdx.x == 0) counts[row] = 0;
        return;
    }
    const float w = (float)rows[3 * row + 1], h = (float)rows[3 * row + 2];
    for (int n = threadIdx.x; n < classes; n += 256) v[n] = logits[(size_t)clip * classes + n];
    __syncthreads();
    for (int n = threadIdx.x; n < classes; n += 256) {
        const float x = v[n];
        int rank = 0, m = 0;
        for (; m + 8 <= classes && rank < k; m += 8)      // eight independent LDS reads per check (the scan is latency-bound)
#pragma unroll
            for (int j = 0; j < 8; ++j) rank += clip_above(v[m + j], m + j, x, n) ? 1 : 0;
        for (; m < classes && rank < k; ++m) rank += clip_above(v[m], m, x, n) ? 1 : 0;
        if (rank < k) {
            const size_t o = (size_t)row * max_det + rank;
            scores[o] = x;
            cls[o] = n;
            *reinterpret_cast<float4 *>(boxes + 4 * o) = make_float4(0.f, 0.f, w, h);
        }
    }
    if (threadIdx.x == 0) counts[row] = k;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// K_stem, K_mean, K_head and K_post serve the other plans too (rva_clip3d.hip and rva_resnet.hip launch them through these;
// declared in rva_internal.h).
int rva_clip_stem_prepare(rva_ctx *ctx)
{
    if (rva_func_smem((const void *)k_clip_stem, STEM_LDS) != hipSuccess)
        return rva_fail(ctx, RVA_ERR_HIP, "clip plan: cannot raise the stem kernel's LDS limit");
    return RVA_OK;
}

int rva_clip_stem_launch(rva_ctx *ctx, const float *frames, const int32_t *frame_index, const float *w1, const float *b1, float *pooled,
                         int H, int W, int n_frames, hipStream_t st)
{
    int Hc, Wc, Hp, Wp;
    rva_stem_maps(H, W, &Hc, &Wc, &Hp, &Wp);
    const int tiles_x = rva_ceil_div(Wp, PT);
    k_clip_stem<<<dim3(tiles_x * rva_ceil_div(Hp, PT), n_frames), STEM_THREADS, STEM_LDS, st>>>(frames, frame_index, w1, b1, pooled, H, W,
                                                                                                Hc, Wc, Hp, Wp, tiles_x);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_clip_mean_launch(rva_ctx *ctx, const float *partial, int tiles, float n, float *feat, int rows, int channels, hipStream_t st)
{
    if (channels < 1 || channels > 256) return rva_fail(ctx, RVA_ERR_ARG, "rva_clip_mean_launch: %d channels, one block holds 1..256", channels);
    k_clip_mean<<<rows, channels, 0, st>>>(partial, tiles, n, feat);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_clip_head_prepare(rva_ctx *ctx, int hidden)
{
    if (rva_func_smem((const void *)k_clip_head, (size_t)hidden * sizeof(float)) != hipSuccess)
        return rva_fail(ctx, RVA_ERR_HIP, "clip plan: cannot raise the head kernel's LDS limit");
    return RVA_OK;
}

int rva_clip_head_launch(rva_ctx *ctx, const float *x, const float *wh, const float *bh, float *logits, int hidden, int classes,
                         int n_clips, hipStream_t st)
{
    k_clip_head<<<dim3(rva_ceil_div(classes, 256), n_clips), 256, (size_t)hidden * sizeof(float), st>>>(x, wh, bh, logits, hidden, classes);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_clip_post_prepare(rva_ctx *ctx, int classes)
{
    if (rva_func_smem((const void *)k_clip_post, (size_t)classes * sizeof(float)) != hipSuccess)
        return rva_fail(ctx, RVA_ERR_HIP, "clip plan: cannot raise the post kernel's LDS limit");
    return RVA_OK;
}

int rva_clip_post_launch(rva_ctx *ctx, const char *who, const float *logits, int classes, int k, const int32_t *rows, int n_rows,
                         int max_det, float *scores, int32_t *cls, float *boxes, int32_t *counts, hipStream_t st)
{
    if (k < 1 || k > classes || !logits || !rows || n_rows < 1 || max_det < k || !scores || !cls || !counts || !boxes || ((uintptr_t)boxes & 15))
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad argument (n_rows >= 1, max_det >= %d, 16-byte aligned boxes)", who, k);
    k_clip_post<<<n_rows, 256, (size_t)classes * sizeof(float), st>>>(logits, classes, rows, k, max_det, scores, cls, boxes, counts);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_clip_stage_copy(rva_ctx *ctx, const char *who, int stage, int n, const char *items, const void *src, size_t esize,
                        const char *unit, int64_t count, int64_t rows, int64_t row_elems, int64_t pitch_elems, void *dst,
                        int64_t dst_elems, int64_t *n_elems, hipStream_t st)
{
    if (n_elems) *n_elems = count;
    if (!dst) return RVA_OK;
    if (dst_elems < count)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: dst holds %lld %s, stage %d of %d %s has %lld", who, (long long)dst_elems, unit, stage,
                        n, items, (long long)count);
    if (rows) {
        const size_t width = (size_t)row_elems * esize;
        RVA_HIP(ctx, hipMemcpy2DAsync(dst, width, src, (size_t)pitch_elems * esize, width, (size_t)rows, hipMemcpyDeviceToDevice, st));
    } else {
        RVA_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)count * esize, hipMemcpyDeviceToDevice, st));
    }
    return RVA_OK;
}

int rva_plan_fits(rva_ctx *ctx, const char *who, size_t need, const char *shape)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b)
        return rva_fail(ctx, RVA_ERR_CAPACITY, "%s: the workspace for %s needs %zu MB, the device has %zu MB free", who, shape,
                        need >> 20, free_b >> 20);
    return RVA_OK;
}

// The fp32 plan: the host plan of rva_clip_host.h over this file's kernels.  The weights stay as they arrive.
struct rva_cnnlstm_plan : rva_cl_plan<float> {
    static constexpr bool REFUSE_LARGE = false;
    static constexpr auto stem_prepare = rva_clip_stem_prepare;
    static constexpr auto stem = rva_clip_stem_launch;
    static constexpr auto xproj = k_clip_xproj;
    static constexpr auto lstm = k_clip_lstm;

    // conv2: [co][ci][ky][kx] -> [co][tap][ci]; layer 2: [W_ih2 | W_hh2] -> [4h][2h]
    static const char *pack(const rva_cnnlstm_desc &d, const rva_cnnlstm_weights &wt, rva_cl_weights<float> &w)
    {
        const int h = d.hidden, G4 = 4 * h;
        w.w1.assign(wt.conv1_w, wt.conv1_w + (size_t)C1 * 3 * K1 * K1);
        w.w2 = rva_pack_taps_major(wt.conv2_w, C2, C1);
        w.wih1.assign(wt.w_ih1, wt.w_ih1 + (size_t)G4 * C2);
        w.whh1.assign(wt.w_hh1, wt.w_hh1 + (size_t)G4 * h);
        w.wl2.resize((size_t)G4 * 2 * h);
        for (int r = 0; r < G4; ++r)
            for (int k = 0; k < h; ++k) {
                w.wl2[(size_t)r * 2 * h + k] = wt.w_ih2[(size_t)r * h + k];
                w.wl2[(size_t)r * 2 * h + h + k] = wt.w_hh2[(size_t)r * h + k];
            }
        return nullptr;
    }

    void conv2(int nf, hipStream_t st)
    {
        k_clip_conv2<<<dim3(g.conv2_tiles, nf), 256, 0, st>>>(pooled, w2, b2, partial, g.Hp, g.Wp, g.conv2_tiles);
    }
};

extern "C" {

int rva_cnnlstm_plan_create(rva_ctx *ctx, const rva_cnnlstm_desc *desc, const rva_cnnlstm_weights *wt, rva_cnnlstm_plan **out)
{
    return rva_cl_create(ctx, "rva_cnnlstm_plan_create", desc, wt, out);
}

void rva_cnnlstm_plan_destroy(rva_cnnlstm_plan *p) { rva_cl_destroy(p); }

int rva_cnnlstm_plan_info(const rva_cnnlstm_plan *p, int32_t *pooled_h, int32_t *pooled_w, int32_t *conv2_tiles, int32_t *n_launches)
{
    return rva_cl_info(p, pooled_h, pooled_w, conv2_tiles, n_launches);
}

int rva_cnnlstm_plan_run(rva_cnnlstm_plan *p, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                         rva_stream_t stream)
{
    return rva_cl_run(p, "rva_cnnlstm_plan_run", frames, frame_index, n_clips, logits, stream);
}

int rva_cnnlstm_plan_run_post(rva_cnnlstm_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                              void *cls, void *boxes, void *counts, rva_stream_t stream)
{
    return rva_cl_run_post(p, "rva_cnnlstm_plan_run_post", logits, rows, n_rows, max_det, scores, cls, boxes, counts, stream);
}

int rva_cnnlstm_plan_stage(rva_cnnlstm_plan *p, int stage, int n_clips, void *dst, int64_t dst_floats, int64_t *n_floats,
                           rva_stream_t stream)
{
    return rva_cl_stage(p, "rva_cnnlstm_plan_stage", stage, n_clips, dst, dst_floats, n_floats, stream);
}

}  // extern "C"
