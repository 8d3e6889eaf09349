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
#include "rva_internal.h"
#include "rva_mfma_f32.h"

#include <algorithm>

namespace {

constexpr int C1 = 64, C2 = 128, K1 = 7;                  // stem widths of the architecture
constexpr int PT = 8;                                      // pooled tile (PT x PT) of K_stem
constexpr int CT = 2 * PT + 1;                             // conv rows of that tile, pool halo included (17)
constexpr int CTW = CT + 1;                                // conv columns (18: pairs of adjacent outputs per thread)
constexpr int IT = 2 * (CT - 1) + K1;                      // input rows of the tile (39)
constexpr int ITW = 2 * (CTW - 1) + K1 + 1;                // input columns, padded (42)
constexpr int STEM_THREADS = 512;
constexpr size_t STEM_LDS = (size_t)(CT * CTW * C1 + 3 * IT * ITW) * sizeof(float);
constexpr int LSTM_U = 4, LSTM_S = 16, LSTM_G = 8;         // units per block, k-slices, clips per pass
constexpr int LSTM_R = 4 * LSTM_U;                         // gate rows per block
constexpr int MAX_HIDDEN = 1024, MAX_T = 64, MAX_CLASSES = RVA_PLAN_MAX_CLASSES;

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
// K_xproj.  Block = (256 gate rows, one clip): gx[clip][t][row] = (sum_k W_ih1[row][k] * feat[t][k], k = 0..127 in order) + b1[row].
__global__ void __launch_bounds__(256) k_clip_xproj(const float *feat_g, const float *wih1, const float *b1, float *gx, int T, int G4)
{
    extern __shared__ float feat[];                        // [T][C2]
    const int clip = blockIdx.y;
    for (int i = threadIdx.x; i < T * C2; i += 256) feat[i] = feat_g[(size_t)clip * T * C2 + i];
    __syncthreads();
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= G4) return;
    float w[C2];
    const float4 *wr = reinterpret_cast<const float4 *>(wih1 + (size_t)row * C2);
#pragma unroll
    for (int q = 0; q < C2 / 4; ++q) {
        const float4 v = wr[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    const float b = b1[row];
    for (int t = 0; t < T; ++t) {
        const float *x = feat + t * C2;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < C2; ++k) s = fmaf(w[k], x[k], s);
        gx[((size_t)clip * T + t) * G4 + row] = s + b;
    }
}

// ---------------------------------------------------------------------------------------------------
// K_lstm, launch s: blockIdx.y = 0 -> layer 1 at step s (s < T), blockIdx.y = 1 -> layer 2 at step s-1 (s >= 1).  Block = units
// [u0, u0+4) x all four gates (16 rows) x every clip, eight clips per pass.  Layer 1: x = h1[s-1] (zero at s = 0), W = W_hh1
// [4h][h], base = gx[clip][s][row].  Layer 2: x = [h1[s-1], h2[s-2]] (h2 zero at step 0), W = [W_ih2 | W_hh2] [4h][2h], base =
// b2[row].  Gate pre-activation = base + sum over the 16 k-slices in order of (slice sigma: k = sigma, sigma+16, ... in order).
// Cell: sigmoid(x) = 1 / (1 + expf(-x)), tanh(x) = 1 - 2 / (expf(2x) + 1); c = f*c + i*g, h = o*tanh(c) (c = 0 at step 0).
// h1 / h2 are [T][cap][hidden]: launch s writes h1[s] and h2[s-1], and reads only h1[s-1] and h2[s-2].
__global__ void __launch_bounds__(256) k_clip_lstm(int s, int T, int hidden, int n_clips, int cap, const float *whh1, const float *w2,
                                                   const float *gx, const float *b2, float *h1, float *h2, float *c1, float *c2)
{
    extern __shared__ float lds[];
    const int layer = blockIdx.y;
    if ((layer == 0 && s >= T) || (layer == 1 && s == 0)) return;
    const int step = layer == 0 ? s : s - 1;
    const int K = layer == 0 ? hidden : 2 * hidden;
    const int G4 = 4 * hidden;
    float *xs = lds;                                       // [LSTM_G][K]
    float *part = xs + LSTM_G * K;                         // [LSTM_R][LSTM_S][LSTM_G]
    float *gates = part + LSTM_R * LSTM_S * LSTM_G;        // [LSTM_R][LSTM_G]
    const int u0 = blockIdx.x * LSTM_U;
    const int rho = threadIdx.x / LSTM_S, sig = threadIdx.x % LSTM_S;
    const int ju = rho % LSTM_U, gate = rho / LSTM_U;
    const bool rv = u0 + ju < hidden;
    const int grow = gate * hidden + (rv ? u0 + ju : 0);
    const float *W = (layer == 0 ? whh1 : w2) + (size_t)grow * K;
    const float *hprev1 = step >= 1 || layer == 1 ? h1 + (size_t)(layer == 0 ? step - 1 : step) * cap * hidden : nullptr;
    const float *hprev2 = layer == 1 && step >= 1 ? h2 + (size_t)(step - 1) * cap * hidden : nullptr;
    float *cst = layer == 0 ? c1 : c2;
    float *hout = (layer == 0 ? h1 : h2) + (size_t)step * cap * hidden;
    for (int b0 = 0; b0 < n_clips; b0 += LSTM_G) {
        __syncthreads();
        for (int i = threadIdx.x; i < LSTM_G * K; i += 256) {
            const int g = i / K, k = i % K, b = b0 + g;
            float v = 0.f;
            if (b < n_clips) {
                if (k < hidden) v = hprev1 ? hprev1[(size_t)b * hidden + k] : 0.f;
                else v = hprev2 ? hprev2[(size_t)b * hidden + k - hidden] : 0.f;
            }
            xs[i] = v;
        }
        __syncthreads();
        float acc[LSTM_G];
#pragma unroll
        for (int g = 0; g < LSTM_G; ++g) acc[g] = 0.f;
        for (int k = sig; k < K; k += LSTM_S) {
            const float wv = W[k];
#pragma unroll
            for (int g = 0; g < LSTM_G; ++g) acc[g] = fmaf(wv, xs[g * K + k], acc[g]);
        }
#pragma unroll
        for (int g = 0; g < LSTM_G; ++g) part[(rho * LSTM_S + sig) * LSTM_G + g] = acc[g];
        __syncthreads();
        if (threadIdx.x < LSTM_R * LSTM_G) {
            const int rr = threadIdx.x / LSTM_G, g = threadIdx.x % LSTM_G, b = b0 + g;
            const int gr = (rr / LSTM_U) * hidden + u0 + rr % LSTM_U;
            float v = 0.f;
            if (b < n_clips && u0 + rr % LSTM_U < hidden) {
                v = layer == 0 ? gx[((size_t)b * T + step) * G4 + gr] : b2[gr];
#pragma unroll
                for (int q = 0; q < LSTM_S; ++q) v = v + part[(rr * LSTM_S + q) * LSTM_G + g];
            }
            gates[rr * LSTM_G + g] = v;
        }
        __syncthreads();
        if (threadIdx.x < LSTM_U * LSTM_G) {
            const int j = threadIdx.x / LSTM_G, g = threadIdx.x % LSTM_G, b = b0 + g, u = u0 + j;
            if (b < n_clips && u < hidden) {
                const float gi = gates[(0 * LSTM_U + j) * LSTM_G + g], gf = gates[(1 * LSTM_U + j) * LSTM_G + g];
                const float gg = gates[(2 * LSTM_U + j) * LSTM_G + g], go = gates[(3 * LSTM_U + j) * LSTM_G + g];
                const float i_ = 1.f / (1.f + expf(-gi)), f_ = 1.f / (1.f + expf(-gf)), o_ = 1.f / (1.f + expf(-go));
                const float g_ = 1.f - 2.f / (expf(2.f * gg) + 1.f);
                const float cp = step == 0 ? 0.f : cst[(size_t)b * hidden + u];
                const float c = f_ * cp + i_ * g_;
                cst[(size_t)b * hidden + u] = c;
                hout[(size_t)b * hidden + u] = o_ * (1.f - 2.f / (expf(2.f * c) + 1.f));
            }
        }
    }
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

size_t lstm_lds(int hidden) { return (size_t)(LSTM_G * 2 * hidden + LSTM_R * LSTM_S * LSTM_G + LSTM_R * LSTM_G) * sizeof(float); }

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

struct rva_cnnlstm_plan {
    rva_ctx *ctx = nullptr;
    rva_cnnlstm_desc d{};
    int Hc = 0, Wc = 0, Hp = 0, Wp = 0, stem_tiles_x = 0, stem_tiles = 0, conv2_tiles = 0;
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;                 // stem
    float *wih1 = nullptr, *bl1 = nullptr, *whh1 = nullptr, *wl2 = nullptr, *bl2 = nullptr, *wh = nullptr, *bh = nullptr;
    float *pooled = nullptr, *partial = nullptr, *feat = nullptr, *gx = nullptr, *h1 = nullptr, *h2 = nullptr, *c1 = nullptr, *c2 = nullptr;
    rva_dev_arena mem;
};

extern "C" {

int rva_cnnlstm_plan_create(rva_ctx *ctx, const rva_cnnlstm_desc *desc, const rva_cnnlstm_weights *wt, rva_cnnlstm_plan **out)
{
    if (!ctx || !desc || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_plan_create: null argument");
    *out = nullptr;
    const rva_cnnlstm_desc d = *desc;
    if (d.height < 2 || d.width < 2 || d.frames < 1 || d.frames > MAX_T || d.hidden < 1 || d.hidden > MAX_HIDDEN || d.classes < 1 ||
        d.classes > MAX_CLASSES || d.max_clips < 1)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_plan_create: bad descriptor (frames 1..%d, hidden 1..%d, classes 1..%d, "
                        "max_clips >= 1)", MAX_T, MAX_HIDDEN, MAX_CLASSES);
    if (!wt->conv1_w || !wt->conv1_b || !wt->conv2_w || !wt->conv2_b || !wt->w_ih1 || !wt->b1 || !wt->w_hh1 || !wt->w_ih2 ||
        !wt->w_hh2 || !wt->b2 || !wt->head_w || !wt->head_b)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_plan_create: every weight array is required");
    // no rva_plan_fits and no max_clips * frames <= 65535 here, unlike rva_cnnlstm_f16_plan_create: this entry has never refused
    // either, and a new refusal is a change of behaviour that wants its own change
    auto *p = new rva_cnnlstm_plan();
    p->ctx = ctx;
    p->d = d;
    rva_stem_maps(d.height, d.width, &p->Hc, &p->Wc, &p->Hp, &p->Wp);
    p->stem_tiles_x = rva_ceil_div(p->Wp, PT);
    p->stem_tiles = p->stem_tiles_x * rva_ceil_div(p->Hp, PT);
    p->conv2_tiles = rva_ceil_div(p->Hp * p->Wp, 256);
    const int h = d.hidden, G4 = 4 * h, T = d.frames;
    const size_t nf = (size_t)d.max_clips * T;
    // conv2: [co][ci][ky][kx] -> [co][tap][ci]; layer 2: [W_ih2 | W_hh2] -> [4h][2h]
    const std::vector<float> w2 = rva_pack_taps_major(wt->conv2_w, C2, C1);
    std::vector<float> wl2((size_t)G4 * 2 * h);
    for (int r = 0; r < G4; ++r)
        for (int k = 0; k < h; ++k) {
            wl2[(size_t)r * 2 * h + k] = wt->w_ih2[(size_t)r * h + k];
            wl2[(size_t)r * 2 * h + h + k] = wt->w_hh2[(size_t)r * h + k];
        }
    int rc = RVA_OK;
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    step(p->mem.upload(ctx, &p->w1, wt->conv1_w, (size_t)C1 * 3 * K1 * K1));
    step(p->mem.upload(ctx, &p->b1, wt->conv1_b, C1));
    step(p->mem.upload(ctx, &p->w2, w2.data(), w2.size()));
    step(p->mem.upload(ctx, &p->b2, wt->conv2_b, C2));
    step(p->mem.upload(ctx, &p->wih1, wt->w_ih1, (size_t)G4 * C2));
    step(p->mem.upload(ctx, &p->bl1, wt->b1, G4));
    step(p->mem.upload(ctx, &p->whh1, wt->w_hh1, (size_t)G4 * h));
    step(p->mem.upload(ctx, &p->wl2, wl2.data(), wl2.size()));
    step(p->mem.upload(ctx, &p->bl2, wt->b2, G4));
    step(p->mem.upload(ctx, &p->wh, wt->head_w, (size_t)d.classes * h));
    step(p->mem.upload(ctx, &p->bh, wt->head_b, d.classes));
    step(p->mem.alloc(ctx, &p->pooled, nf * p->Hp * p->Wp * C1));
    step(p->mem.alloc(ctx, &p->partial, nf * p->conv2_tiles * C2));
    step(p->mem.alloc(ctx, &p->feat, nf * C2));
    step(p->mem.alloc(ctx, &p->gx, nf * G4));
    step(p->mem.alloc(ctx, &p->h1, (size_t)T * d.max_clips * h));
    step(p->mem.alloc(ctx, &p->h2, (size_t)T * d.max_clips * h));
    step(p->mem.alloc(ctx, &p->c1, (size_t)d.max_clips * h));
    step(p->mem.alloc(ctx, &p->c2, (size_t)d.max_clips * h));
    if (rc == RVA_OK) rc = rva_clip_stem_prepare(ctx);
    if (rc == RVA_OK && rva_func_smem((const void *)k_clip_lstm, lstm_lds(h)) != hipSuccess)
        rc = rva_fail(ctx, RVA_ERR_HIP, "rva_cnnlstm_plan_create: cannot raise the LSTM kernel's LDS limit");
    if (rc == RVA_OK) rc = rva_clip_head_prepare(ctx, h);
    if (rc == RVA_OK) rc = rva_clip_post_prepare(ctx, d.classes);
    if (rc != RVA_OK) {
        rva_cnnlstm_plan_destroy(p);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

void rva_cnnlstm_plan_destroy(rva_cnnlstm_plan *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

int rva_cnnlstm_plan_info(const rva_cnnlstm_plan *p, int32_t *pooled_h, int32_t *pooled_w, int32_t *conv2_tiles, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    if (pooled_h) *pooled_h = p->Hp;
    if (pooled_w) *pooled_w = p->Wp;
    if (conv2_tiles) *conv2_tiles = p->conv2_tiles;
    if (n_launches) *n_launches = 4 + (p->d.frames + 1) + 1;
    return RVA_OK;
}

int rva_cnnlstm_plan_run(rva_cnnlstm_plan *p, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                         rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_plan_run: bad argument (n_clips %d, capacity %d)", n_clips, p->d.max_clips);
    const hipStream_t st = (hipStream_t)stream_;
    const int T = p->d.frames, h = p->d.hidden, G4 = 4 * h, nf = n_clips * T;
    int rc = rva_clip_stem_launch(ctx, (const float *)frames, frame_index, p->w1, p->b1, p->pooled, p->d.height, p->d.width, nf, st);
    if (rc != RVA_OK) return rc;
    k_clip_conv2<<<dim3(p->conv2_tiles, nf), 256, 0, st>>>(p->pooled, p->w2, p->b2, p->partial, p->Hp, p->Wp, p->conv2_tiles);
    RVA_HIP(ctx, hipGetLastError());
    rc = rva_clip_mean_launch(ctx, p->partial, p->conv2_tiles, (float)(p->Hp * p->Wp), p->feat, nf, C2, st);
    if (rc != RVA_OK) return rc;
    k_clip_xproj<<<dim3(rva_ceil_div(G4, 256), n_clips), 256, (size_t)T * C2 * sizeof(float), st>>>(
        p->feat, p->wih1, p->bl1, p->gx, T, G4);
    RVA_HIP(ctx, hipGetLastError());
    for (int s = 0; s <= T; ++s) {
        k_clip_lstm<<<dim3(rva_ceil_div(h, LSTM_U), 2), 256, lstm_lds(h), st>>>(s, T, h, n_clips, p->d.max_clips, p->whh1, p->wl2,
                                                                                p->gx, p->bl2, p->h1, p->h2, p->c1, p->c2);
        RVA_HIP(ctx, hipGetLastError());
    }
    return rva_clip_head_launch(ctx, p->h2 + (size_t)(T - 1) * p->d.max_clips * h, p->wh, p->bh, (float *)logits, h, p->d.classes,
                                n_clips, st);
}

int rva_cnnlstm_plan_run_post(rva_cnnlstm_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                              void *cls, void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, "rva_cnnlstm_plan_run_post", (const float *)logits, p->d.classes, std::min(5, p->d.classes), rows, n_rows, max_det,
                                (float *)scores, (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  h1 / h2 keep max_clips rows per
// step, so fewer clips than the capacity are T rows of n_clips * hidden out of a pitch of max_clips * hidden: one 2D copy.
int rva_cnnlstm_plan_stage(rva_cnnlstm_plan *p, int stage, int n_clips, void *dst, int64_t dst_floats, int64_t *n_floats,
                           rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_plan_stage: bad argument (n_clips %d, capacity %d)", n_clips, p->d.max_clips);
    const int64_t T = p->d.frames, h = p->d.hidden, nf = (int64_t)n_clips * T;
    const float *src = nullptr;
    int64_t count = 0;
    switch (stage) {
    case RVA_CNNLSTM_STAGE_POOLED: src = p->pooled; count = nf * p->Hp * p->Wp * C1; break;
    case RVA_CNNLSTM_STAGE_PARTIAL: src = p->partial; count = nf * p->conv2_tiles * C2; break;
    case RVA_CNNLSTM_STAGE_FEAT: src = p->feat; count = nf * C2; break;
    case RVA_CNNLSTM_STAGE_GX: src = p->gx; count = nf * 4 * h; break;
    case RVA_CNNLSTM_STAGE_H1: src = p->h1; count = nf * h; break;
    case RVA_CNNLSTM_STAGE_H2: src = p->h2; count = nf * h; break;
    default: return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_plan_stage: unknown stage %d", stage);
    }
    const bool rows = (stage == RVA_CNNLSTM_STAGE_H1 || stage == RVA_CNNLSTM_STAGE_H2) && n_clips < p->d.max_clips;
    return rva_clip_stage_copy(ctx, "rva_cnnlstm_plan_stage", stage, n_clips, "clips", src, sizeof(float), "floats", count, rows ? T : 0,
                               n_clips * h, p->d.max_clips * h, dst, dst_floats, n_floats, (hipStream_t)stream_);
}

}  // extern "C"
