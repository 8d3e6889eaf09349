// 3D-CNN clip network (the reference's 3D-CNN head, scripts/convert_temporal_model_to_onnx.py:91-121) as one plan object, in fp32
// (rva_cnn3d_plan_*) and for `half: true` (rva_cnn3d_f16_plan_*, engine "clip3d-f16"):
//
//   per clip [3,T,H,W]: Conv3d(3,64,3,p1)+BN+ReLU -> MaxPool3d((1,2,2)) -> Conv3d(64,128,3,p1)+BN+ReLU -> MaxPool3d(2)
//                       -> Conv3d(128,256,3,p1)+BN+ReLU -> mean over T,H,W -> Linear(256 -> classes) -> top-k (k = min(5, classes))
//
// The two precisions are ONE network, one set of launches and one block and wave decomposition, written once over the element
// type E of the frames, the conv2 / conv3 weights and the stored activations act1 / act2.  BatchNorm is folded by the caller in
// float64 and rounded once to fp32; activations are channels-last ([T][H][W][C]).  Every sum accumulates in fp32 in ONE fixed
// order that depends neither on the number of clips, nor on a clip's position in the batch, nor on the launch mode -- no split-K
// whose order follows the grid and no float atomics -- so logits are bit-identical across batch sizes, clip positions, an
// index-table permutation of the ring, eager launches and hipGraph replay.  The pools follow torch (floor, no padding): trailing
// odd rows, columns and frames are dropped and the convolution outputs that only feed them are not computed.  A max commutes
// exactly with the monotonic "+ bias, ReLU", so the pools take the max of the raw sums first.
//
// E = _Float16: the ring holds planar fp16 frames [3][H][W]; create rounds each convolution weight once to fp16 (round to nearest
// even; a value that does not stay finite is refused).  Biases, head weight and head bias stay fp32.  act1 / act2 take ONE
// rounding to fp16, of ReLU(max of the raw fp32 sums + bias); conv3's tile partials, the mean, the head and the logits are fp32.
//
// The launches of one pass (c3d_run):
//
//   K_conv1  conv1 + 2x2 spatial max pool + bias + ReLU, 8x8 pooled tile of one frame per block; reads the planar frames straight
//            from the caller's ring through the device table of frame indices (frame t of clip b and its temporal neighbours
//            are entries b*T + t - 1 .. b*T + t + 1; zero outside the clip).  VALU fmaf, taps in the checkpoint's (ci, kt, ky,
//            kx) order, on fp32 values in LDS and registers: fp16 frames are widened on the way into LDS (exact) and the fp16
//            plan's weights are the fp16-rounded values held as fp32, so its chain adds exact products.  Frame rows are read
//            element by element: nothing is assumed about the alignment of a row (odd widths).  Writes [T][H/2][W/2][64].
//   K_conv2  27 taps x 64 channels on the MFMA core of the element type (c3d_taps), which defines the reduction order: the exact
//            fp32-input core of rva_mfma_f32.h, or v_mfma_f32_32x32x16_f16 with a step's weights staged through LDS once per
//            block (f16_conv_taps_wlds).  A block owns 32 whole 2x2x2 pool groups, so the max pool + bias + ReLU run in the
//            epilogue and the unpooled 128-channel volume is never written.  Writes [T/2][H/4][W/4][128].
//   K_conv3  27 taps x 128 channels, same core; bias + ReLU, then the tile's per-channel sum (positions in tile order): the
//            256-channel volume is never written.  Writes fp32 tile partials.
//   K_mean   a clip's tile partials reduced in tile order and divided by T'*H'*W': the mean kernel of rva_clip.hip.
//   K_head   Linear: the head kernel of rva_clip.hip (one thread per class, k in order).
//   K_post   (c3d_run_post) the top-k kernel of rva_clip.hip.
#include "rva_mfma_f16.h"
#include "rva_plan_topo.h"

#include <type_traits>

namespace {

constexpr int C1 = C3D_C1, C2 = C3D_C2, C3 = C3D_C3;       // widths of the architecture
constexpr int TAPS = C3D_TAPS;
constexpr int PT = C3D_PT;                                 // pooled tile (PT x PT) of K_conv1
constexpr int IT = 2 * PT + 2;                             // input rows / columns of that tile (18)
constexpr int ITW = IT + 2;                                // padded LDS row (20)
constexpr int CONV1_THREADS = 256;
constexpr int MT = 2, NT = 4;                              // 32x32 MFMA tiles of a wave: 64 positions x 128 channels
constexpr int GROUPS = C3D_GROUPS;                         // pool groups (of 8 conv positions) of a K_conv2 block

// the 27 taps x CIN channels of a wave's 64 positions, on the core of the element type
template <int CIN>
__device__ __forceinline__ void c3d_taps(f32x16 (&acc)[MT][NT], const float *in, const float *w, const int (&pt)[MT], const int (&py)[MT],
                                         const int (&px)[MT], const bool (&pv)[MT], int T, int H, int W)
{
    f32_conv_taps<CIN, 3>(acc, in, w, pt, py, px, pv, T, H, W);
}

template <int CIN>
__device__ __forceinline__ void c3d_taps(f32x16 (&acc)[MT][NT], const _Float16 *in, const _Float16 *w, const int (&pt)[MT],
                                         const int (&py)[MT], const int (&px)[MT], const bool (&pv)[MT], int T, int H, int W)
{
    f16_conv_taps_wlds<CIN, 3>(acc, in, w, pt, py, px, pv, T, H, W);
}

// ---------------------------------------------------------------------------------------------------
// K_conv1.  Thread = output channel (tid & 63) x a wave-uniform pooled position, so the input reads are LDS broadcasts and each
// thread keeps its 81 weights in registers.  The four conv outputs under a pooled position share one 4x4 input window per
// (channel, frame).  Sum of a conv output: fmaf chain from 0 over (ci, kt, ky, kx) in order; then max of the four, + bias, ReLU,
// stored as E.
template <class E>
__device__ __forceinline__ void c3d_conv1(const E *ring, const int32_t *frame_index, const float *w1, const float *b1, E *act1, int T,
                                          int H, int W, int H1, int W1, int tiles_x)
{
    __shared__ float xin[3 * 3 * IT * ITW];                // [kt][ci][IT][ITW]
    const int f = blockIdx.y, t = f % T;
    const int py0 = (blockIdx.x / tiles_x) * PT, px0 = (blockIdx.x % tiles_x) * PT;
    const int iy0 = 2 * py0 - 1, ix0 = 2 * px0 - 1;
    for (int kt = 0; kt < 3; ++kt) {
        const int tt = t + kt - 1;
        const bool tv = (unsigned)tt < (unsigned)T;       // block-uniform
        const E *img = tv ? ring + (size_t)frame_index[f + kt - 1] * 3 * H * W : ring;
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
        act1[(((size_t)f * H1 + py) * W1 + px) * C1 + co] = (E)fmaxf(m + bias, 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------
// K_conv2.  Block = 32 pool groups (linear over [T2][H2][W2]) of one clip x all 128 channels; wave = 8 groups = 64 conv positions.
// Row m of a wave's 64: group m >> 3, position (dt, dy, dx) = bits 2, 1, 0 of m & 7 inside it.  C/D map (f32_cd_row): column =
// lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) -- so registers 4j .. 4j+3 of a lane are half a pool group and the other
// lane half holds the rest.  Epilogue: max of the eight raw sums, + bias, ReLU, stored as E.
template <class E>
__device__ __forceinline__ void c3d_conv2(const E *act1, const E *w2, const float *b2, E *act2, int T, int H1, int W1, int T2, int H2,
                                          int W2)
{
    const int clip = blockIdx.y, tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int NG = T2 * H2 * W2;
    const int g0 = tile * GROUPS + wave * (GROUPS / 4);
    const E *in = act1 + (size_t)clip * T * H1 * W1 * C1;
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
    c3d_taps<C1>(acc, in, w2, pt, py, px, pv, T, H1, W1);
    E *out = act2 + (size_t)clip * NG * C2;
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
                if ((j & 1) == h && g < NG) out[(size_t)g * C2 + co] = (E)fmaxf(v + bias, 0.f);
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// K_conv3.  Block = 256 positions (linear over [T2][H2][W2]; four waves of 64) of one clip x 128 of the 256 channels
// (blockIdx.y = channel half).  Epilogue: f32_tile_sum (bias + ReLU, then the tile's per-channel sum), fp32.
template <class E>
__device__ __forceinline__ void c3d_conv3(const E *act2, const E *w3, const float *b3, float *partial, int T2, int H2, int W2, int tiles)
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
    c3d_taps<C2>(acc, act2 + (size_t)clip * P * C2, w3 + (size_t)cb * C2 * TAPS * C2, pt, py, px, pv, T2, H2, W2);
    f32_tile_sum(acc, b3 + cb * C2, m0, P, partial + ((size_t)clip * tiles + tile) * C3 + cb * C2);
}

// The kernels, under the names the traces of the report tools know.
__global__ void __launch_bounds__(CONV1_THREADS) k_c3d_conv1(const float *ring, const int32_t *frame_index, const float *w1,
                                                             const float *b1, float *act1, int T, int H, int W, int H1, int W1,
                                                             int tiles_x)
{
    c3d_conv1(ring, frame_index, w1, b1, act1, T, H, W, H1, W1, tiles_x);
}

__global__ void __launch_bounds__(256) k_c3d_conv2(const float *act1, const float *w2, const float *b2, float *act2, int T, int H1,
                                                   int W1, int T2, int H2, int W2)
{
    c3d_conv2(act1, w2, b2, act2, T, H1, W1, T2, H2, W2);
}

__global__ void __launch_bounds__(256) k_c3d_conv3(const float *act2, const float *w3, const float *b3, float *partial, int T2, int H2,
                                                   int W2, int tiles)
{
    c3d_conv3(act2, w3, b3, partial, T2, H2, W2, tiles);
}

__global__ void __launch_bounds__(CONV1_THREADS) k_c3d16_conv1(const _Float16 *ring, const int32_t *frame_index, const float *w1,
                                                               const float *b1, _Float16 *act1, int T, int H, int W, int H1, int W1,
                                                               int tiles_x)
{
    c3d_conv1(ring, frame_index, w1, b1, act1, T, H, W, H1, W1, tiles_x);
}

__global__ void __launch_bounds__(256) k_c3d16_conv2(const _Float16 *act1, const _Float16 *w2, const float *b2, _Float16 *act2, int T,
                                                     int H1, int W1, int T2, int H2, int W2)
{
    c3d_conv2(act1, w2, b2, act2, T, H1, W1, T2, H2, W2);
}

__global__ void __launch_bounds__(256) k_c3d16_conv3(const _Float16 *act2, const _Float16 *w3, const float *b3, float *partial, int T2,
                                                     int H2, int W2, int tiles)
{
    c3d_conv3(act2, w3, b3, partial, T2, H2, W2, tiles);
}

// The plan over the element type E.  The fp32 plan keeps the weights as they arrive; the fp16 plan rounds them.
template <class E>
struct c3d_plan {
    typedef E elem;
    rva_ctx *ctx = nullptr;
    rva_cnn3d_desc d{};
    rva_c3d_geom g{};
    float *w1 = nullptr, *b1 = nullptr, *b2 = nullptr, *b3 = nullptr, *wh = nullptr, *bh = nullptr;
    E *w2 = nullptr, *w3 = nullptr, *act1 = nullptr, *act2 = nullptr;
    float *partial = nullptr, *feat = nullptr;
    rva_dev_arena mem;
};

bool c3d_round(const float *src, size_t n, std::vector<float> &dst) { dst.assign(src, src + n); return true; }
bool c3d_round(const float *src, size_t n, std::vector<_Float16> &dst) { return rva_round_f16(src, n, dst); }

}  // namespace

// the two handles of include/rva.h: the plan of their element type and its three kernels
struct rva_cnn3d_plan : c3d_plan<float> {
    static constexpr auto conv1 = k_c3d_conv1;
    static constexpr auto conv2 = k_c3d_conv2;
    static constexpr auto conv3 = k_c3d_conv3;
};

struct rva_cnn3d_f16_plan : c3d_plan<_Float16> {
    static constexpr auto conv1 = k_c3d16_conv1;
    static constexpr auto conv2 = k_c3d16_conv2;
    static constexpr auto conv3 = k_c3d16_conv3;
};

namespace {

template <class P>
void c3d_destroy(P *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

template <class P>
int c3d_create(rva_ctx *ctx, const char *who, const rva_cnn3d_desc *desc, const rva_cnn3d_weights *wt, P **out)
{
    typedef typename P::elem E;
    int rc = rva_c3d_check_args(ctx, who, desc, wt, (void **)out);
    if (rc != RVA_OK) return rc;
    const rva_cnn3d_desc d = *desc;
    std::vector<E> h1, h2, h3;
    const char *bad = !c3d_round(wt->conv1_w, C3D_W1, h1) ? "conv1_w" : !c3d_round(wt->conv2_w, C3D_W2, h2) ? "conv2_w" :
                      !c3d_round(wt->conv3_w, C3D_W3, h3) ? "conv3_w" : nullptr;
    if (bad) return rva_fail(ctx, RVA_ERR_ARG, "%s: a value of %s does not stay finite in fp16", who, bad);
    const std::vector<float> w1f(h1.begin(), h1.end());     // K_conv1 keeps its weights in fp32 registers: the values of E, widened
    const rva_c3d_geom g = rva_c3d_geometry(d);
    const size_t mc = (size_t)d.max_clips;
    const size_t n_act1 = mc * g.elems[RVA_CNN3D_STAGE_ACT1], n_act2 = mc * g.elems[RVA_CNN3D_STAGE_ACT2];
    const size_t n_part = mc * g.elems[RVA_CNN3D_STAGE_PARTIAL], n_feat = mc * g.elems[RVA_CNN3D_STAGE_FEAT];
    const size_t need = (n_act1 + n_act2 + C3D_W2 + C3D_W3) * sizeof(E) +
                        (n_part + n_feat + C3D_W1 + C1 + C2 + C3 + (size_t)d.classes * (C3 + 1)) * sizeof(float);
    char shape[64];
    snprintf(shape, sizeof shape, "%d clips of %d x %d x %d", d.max_clips, d.frames, d.height, d.width);
    rc = rva_plan_fits(ctx, who, need, shape);
    if (rc != RVA_OK) return rc;
    auto *p = new P();
    p->ctx = ctx;
    p->d = d;
    p->g = g;
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    step(p->mem.upload(ctx, &p->w1, w1f.data(), C3D_W1));
    step(p->mem.upload(ctx, &p->b1, wt->conv1_b, C1));
    step(p->mem.upload(ctx, &p->w2, h2.data(), C3D_W2));
    step(p->mem.upload(ctx, &p->b2, wt->conv2_b, C2));
    step(p->mem.upload(ctx, &p->w3, h3.data(), C3D_W3));
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
        c3d_destroy(p);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

template <class P>
int c3d_info(const P *p, int32_t *pool1, int32_t *pool2, int32_t *tiles, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    rva_c3d_info(p->g, pool1, pool2, tiles, n_launches);
    return RVA_OK;
}

template <class P>
int c3d_run(P *p, const char *who, const void *frames, const int32_t *frame_index, int n_clips, void *logits, rva_stream_t stream_)
{
    typedef typename P::elem E;
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad argument (n_clips %d, capacity %d)", who, n_clips, p->d.max_clips);
    const hipStream_t st = (hipStream_t)stream_;
    const rva_c3d_geom &g = p->g;
    P::conv1<<<dim3(g.conv1_tiles, n_clips * g.T), CONV1_THREADS, 0, st>>>((const E *)frames, frame_index, p->w1, p->b1, p->act1, g.T,
                                                                           p->d.height, p->d.width, g.H1, g.W1, g.conv1_tiles_x);
    RVA_HIP(ctx, hipGetLastError());
    P::conv2<<<dim3(g.conv2_tiles, n_clips), 256, 0, st>>>(p->act1, p->w2, p->b2, p->act2, g.T, g.H1, g.W1, g.T2, g.H2, g.W2);
    RVA_HIP(ctx, hipGetLastError());
    P::conv3<<<dim3(g.conv3_tiles, 2, n_clips), 256, 0, st>>>(p->act2, p->w3, p->b3, p->partial, g.T2, g.H2, g.W2, g.conv3_tiles);
    RVA_HIP(ctx, hipGetLastError());
    int rc = rva_clip_mean_launch(ctx, p->partial, g.conv3_tiles, (float)((size_t)g.T2 * g.H2 * g.W2), p->feat, n_clips, C3, st);
    if (rc != RVA_OK) return rc;
    return rva_clip_head_launch(ctx, p->feat, p->wh, p->bh, (float *)logits, C3, p->d.classes, n_clips, st);
}

template <class P>
int c3d_run_post(P *p, const char *who, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores, void *cls,
                 void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, who, (const float *)logits, p->d.classes, std::min(5, p->d.classes), rows, n_rows, max_det,
                                (float *)scores, (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  Every tensor is clip-major; ACT1 / ACT2
// are elements of E, PARTIAL / FEAT fp32, and the counts are element counts ("floats" in the fp32 plan's size error).
template <class P>
int c3d_stage(P *p, const char *who, int stage, int n_clips, void *dst, int64_t dst_elems, int64_t *n_elems, rva_stream_t stream_)
{
    typedef typename P::elem E;
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad argument (n_clips %d, capacity %d)", who, n_clips, p->d.max_clips);
    if (stage < 0 || stage > RVA_CNN3D_STAGE_FEAT) return rva_fail(ctx, RVA_ERR_ARG, "%s: unknown stage %d", who, stage);
    const void *const src[4] = {p->act1, p->act2, p->partial, p->feat};
    const size_t esize = stage <= RVA_CNN3D_STAGE_ACT2 ? sizeof(E) : sizeof(float);
    return rva_clip_stage_copy(ctx, who, stage, n_clips, "clips", src[stage], esize, std::is_same<E, float>::value ? "floats" : "elements",
                               n_clips * p->g.elems[stage], 0, 0, 0, dst, dst_elems, n_elems, (hipStream_t)stream_);
}

}  // namespace

extern "C" {

int rva_cnn3d_plan_create(rva_ctx *ctx, const rva_cnn3d_desc *desc, const rva_cnn3d_weights *wt, rva_cnn3d_plan **out)
{
    return c3d_create(ctx, "rva_cnn3d_plan_create", desc, wt, out);
}

void rva_cnn3d_plan_destroy(rva_cnn3d_plan *p) { c3d_destroy(p); }

int rva_cnn3d_plan_info(const rva_cnn3d_plan *p, int32_t *pool1, int32_t *pool2, int32_t *tiles, int32_t *n_launches)
{
    return c3d_info(p, pool1, pool2, tiles, n_launches);
}

int rva_cnn3d_plan_run(rva_cnn3d_plan *p, const void *frames, const int32_t *frame_index, int n_clips, void *logits, rva_stream_t stream)
{
    return c3d_run(p, "rva_cnn3d_plan_run", frames, frame_index, n_clips, logits, stream);
}

int rva_cnn3d_plan_run_post(rva_cnn3d_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                            void *cls, void *boxes, void *counts, rva_stream_t stream)
{
    return c3d_run_post(p, "rva_cnn3d_plan_run_post", logits, rows, n_rows, max_det, scores, cls, boxes, counts, stream);
}

int rva_cnn3d_plan_stage(rva_cnn3d_plan *p, int stage, int n_clips, void *dst, int64_t dst_floats, int64_t *n_floats, rva_stream_t stream)
{
    return c3d_stage(p, "rva_cnn3d_plan_stage", stage, n_clips, dst, dst_floats, n_floats, stream);
}

int rva_cnn3d_f16_plan_create(rva_ctx *ctx, const rva_cnn3d_desc *desc, const rva_cnn3d_weights *wt, rva_cnn3d_f16_plan **out)
{
    return c3d_create(ctx, "rva_cnn3d_f16_plan_create", desc, wt, out);
}

void rva_cnn3d_f16_plan_destroy(rva_cnn3d_f16_plan *p) { c3d_destroy(p); }

int rva_cnn3d_f16_plan_info(const rva_cnn3d_f16_plan *p, int32_t *pool1, int32_t *pool2, int32_t *tiles, int32_t *n_launches)
{
    return c3d_info(p, pool1, pool2, tiles, n_launches);
}

int rva_cnn3d_f16_plan_run(rva_cnn3d_f16_plan *p, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                           rva_stream_t stream)
{
    return c3d_run(p, "rva_cnn3d_f16_plan_run", frames, frame_index, n_clips, logits, stream);
}

int rva_cnn3d_f16_plan_run_post(rva_cnn3d_f16_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                                void *cls, void *boxes, void *counts, rva_stream_t stream)
{
    return c3d_run_post(p, "rva_cnn3d_f16_plan_run_post", logits, rows, n_rows, max_det, scores, cls, boxes, counts, stream);
}

int rva_cnn3d_f16_plan_stage(rva_cnn3d_f16_plan *p, int stage, int n_clips, void *dst, int64_t dst_elems, int64_t *n_elems,
                             rva_stream_t stream)
{
    return c3d_stage(p, "rva_cnn3d_f16_plan_stage", stage, n_clips, dst, dst_elems, n_elems, stream);
}

}  // extern "C"
