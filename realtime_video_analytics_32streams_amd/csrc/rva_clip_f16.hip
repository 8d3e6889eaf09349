// The CNN-LSTM clip network of rva_clip.hip for `half: true` (engine "clip-f16"): the same network and launches, with fp16 frames,
// fp16 convolution and LSTM weights and an fp16 stored `pooled`, and every sum in fp32.  The numeric contract is clip3d-f16's:
//
//   * input: the detector's ring of planar fp16 frames [3][H][W], read through the device table of frame indices, element by
//     element: nothing is assumed about the alignment of a frame row (odd widths);
//   * weights: conv1 / conv2 arrive with their BatchNorm folded by the caller in float64; rva_cnnlstm_f16_plan_create rounds
//     conv1_w, conv2_w, w_ih1, w_hh1, w_ih2 and w_hh2 once to fp16 (round to nearest even; a value that does not stay finite is
//     refused, naming its array).  The two summed LSTM biases, the conv biases, head weight and head bias stay fp32;
//   * stored activations: `pooled` [n T][Hp][Wp][64] is fp16 with ONE rounding, of ReLU(max of the raw fp32 sums + bias).
//     Everything after conv2 is fp32: tile partials, feat, gx, h1, h2, the cell states, logits and top-5 scores;
//   * every sum accumulates in fp32 in ONE fixed order that depends neither on the number of clips, nor on a clip's position, nor
//     on the launch mode: no split-K that follows the grid and no float atomics, so logits are bit-identical across all of those.
//
//   K_stem   conv1 as an implicit GEMM on v_mfma_f32_32x32x16_f16 with bias + ReLU + the 3x3/s2/p1 max pool in the epilogue; the
//            fp32 stem's tile: 8x8 pooled values per block, their 17x17 conv values (pool halo included) in LDS, -inf at conv
//            positions outside the map.  The block's 39 x 40 x 3 input tile is staged in LDS as fp16.  Reduction order of a conv
//            value: K index k = (ci 7 + ky) 8 + kx, kx padded from 7 to 8, plus one padded row: 22 rows of 8 = 176 = 11 chunks of
//            16, one MFMA per chunk from a zero accumulator, chunks in order; lane half h of chunk c supplies row 2c + h -- eight
//            consecutive fp16 of one input row of the LDS tile against eight weights.  Every padded slot is 0 x 0 (the weight is
//            zero and the input lane is masked to zero), the 147 real products are exact in fp32, and inside the instruction the
//            16 products are added in the hardware's fixed order.  The conv tile is kept in LDS as fp16 of ReLU(sum + bias):
//            rounding, ReLU and + bias are monotone, so the max of the rounded values IS the one rounding of ReLU(max + bias).
//   K_conv2  3x3 conv on rva_mfma_f16.h (9 taps x 4 chunks of 16 channels, its reduction order), block and wave decomposition
//            and epilogue of k_clip_conv2: f32_tile_sum into fp32 tile partials.  The block's weights go through LDS
//            (f16_conv_taps_wlds); RVA_CLIP16_WLDS=0 at plan creation selects the straight form in which every wave loads its
//            own (f16_conv_taps).  Same reduction order: the two are bit-identical.
//   K_xproj  as k_clip_xproj with W_ih1 fp16 in HBM (a thread's row is 16 contiguous 16-byte reads), widened on load.
//   K_lstm   the T + 1 diagonal launches of k_clip_lstm with W_hh1 and [W_ih2 | W_hh2] fp16 in HBM, slice-major (lstm_pack), widened
//            on load.  Both bodies, their reduction orders and the cell are rva_lstm_dev.h's: one text for both precisions.
//   K_mean / K_head / K_post: the kernels of rva_clip.hip.
#include "rva_clip_host.h"
#include "rva_lstm_dev.h"

#include <cmath>

namespace {

constexpr int C1 = CL_C1, C2 = CL_C2, K1 = CL_K1;         // stem widths of the architecture
constexpr int PT = CL_PT;                                  // pooled tile (PT x PT) of K_stem
constexpr int CT = 2 * PT + 1;                             // conv rows / columns of that tile, pool halo included (17)
constexpr int NP = CT * CT;                                // conv positions of the tile (289)
constexpr int IT = 2 * (CT - 1) + K1;                      // input rows of the tile (39)
constexpr int IW = 2 * (CT - 1) + K1 + 1;                  // input columns the MFMA operands read (40: kx padded to 8)
constexpr int ITW = 50;                                    // LDS row of the input tile, in fp16.  Consecutive conv rows are two
                                                           //   input rows = 50 dwords = 18 banks (mod 32) apart, so the 32 lanes of
                                                           //   a 4-byte operand read (17 positions per conv row, stride-2 columns =
                                                           //   consecutive dwords) collide 2-way on at most two banks
constexpr int CS = C1 + 4;                                 // LDS row of a conv position, in fp16 (34 dwords: 8-byte stores of
                                                           //   16 consecutive positions fall on 32 different banks)
constexpr int KROWS = 3 * K1 + 1, KP = KROWS * 8;          // 22 rows of 8 = 176
constexpr int CHUNKS = KP / 16;                            // 11
constexpr int KPS = KP + 8;                                // row of the packed conv1 weights, in fp16, in HBM and in LDS: 92 dwords,
                                                           //   which puts the 16 rows of a ds_read_b128 lane group on 16 different
                                                           //   16-byte slots of the 256-byte bank row
constexpr int STEM_WAVES = 5, STEM_THREADS = 64 * STEM_WAVES, STEM_MT = 2;   // 10 tiles of 32 positions cover 289

static_assert(STEM_WAVES * STEM_MT * 32 >= NP, "the waves cover the conv tile");
static_assert(ITW >= IW && ITW % 2 == 0 && CS % 4 == 0, "dword rows, 8-byte conv stores");
static_assert(C1 * KPS <= NP * CS && (C1 * KPS) % 8 == 0, "the weights fit the conv tile's LDS, in whole 16-byte slots");

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------
// K_stem.  GEMM rows = the 64 output channels (two tiles of 32; a wave keeps all 22 weight operands in registers: the block
// fetches the 23 KB of weights once, into the LDS that later holds the conv tile, and every wave takes its operands from there --
// five waves loading them from L2 each was the kernel's largest cost), GEMM columns =
// conv positions of the tile (ten tiles of 32, two per wave; position m = ly 17 + lx, m >= 289 computed on position 288 and
// dropped).  So register 4j + e of an accumulator is channel 32 ct + 8j + 4h + e of the lane's position: four consecutive channels
// per 8-byte LDS store.
__global__ void __launch_bounds__(STEM_THREADS) k_clip16_stem(const _Float16 *ring, const int32_t *frame_index, const _Float16 *w1,
                                                              const float *b1, _Float16 *pooled, int H, int W, int Hc, int Wc,
                                                              int Hp, int Wp, int tiles_x)
{
    __shared__ __attribute__((aligned(16))) _Float16 xin[3 * IT * ITW];      // [3][IT][ITW]
    __shared__ __attribute__((aligned(16))) _Float16 conv[NP * CS];          // [CT][CT][CS]
    const int f = blockIdx.y;
    const int py0 = (blockIdx.x / tiles_x) * PT, px0 = (blockIdx.x % tiles_x) * PT;
    const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;        // first conv row / column of the tile
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;        // first input row / column
    const _Float16 *img = ring + (size_t)frame_index[f] * 3 * H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    // the weights and the input tile: every load of a thread is issued before its first LDS store (a load-store loop would pay
    // the memory latency once per element)
    constexpr int NWS = C1 * KPS / 8, NWT = (NWS + STEM_THREADS - 1) / STEM_THREADS;
    f16x8 tw[NWT];
#pragma unroll
    for (int j = 0; j < NWT; ++j) {
        const int sl = threadIdx.x + j * STEM_THREADS;
        tw[j] = sl < NWS ? reinterpret_cast<const f16x8 *>(w1)[sl] : f16x8{};
    }
    constexpr int NIN = 3 * IT * IW, NST = (NIN + STEM_THREADS - 1) / STEM_THREADS;
    _Float16 sv[NST];
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = threadIdx.x + j * STEM_THREADS;
        const int c = i / (IT * IW), rr = (i / IW) % IT, q = i % IW;
        const int iy = iy0 + rr, ix = ix0 + q;
        sv[j] = (i < NIN && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) ? img[((size_t)c * H + iy) * W + ix] : (_Float16)0.f;
    }
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = threadIdx.x + j * STEM_THREADS;
        const int c = i / (IT * IW), rr = (i / IW) % IT, q = i % IW;
        if (i < NIN) xin[(c * IT + rr) * ITW + q] = sv[j];
    }
#pragma unroll
    for (int j = 0; j < NWT; ++j) {
        const int sl = threadIdx.x + j * STEM_THREADS;
        if (sl < NWS) reinterpret_cast<f16x8 *>(conv)[sl] = tw[j];
    }
    __syncthreads();
    f16x8 fw[CHUNKS][2];
    int xo[CHUNKS];                                        // LDS offset of the lane's input row of chunk c, from the position's
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) fw[c][ct] = *reinterpret_cast<const f16x8 *>(conv + (ct * 32 + r) * KPS + (2 * c + h) * 8);
        const int row = 2 * c + h < KROWS - 1 ? 2 * c + h : KROWS - 2;       // the padded row reads row 20's input and masks it
        xo[c] = ((row / K1) * IT + row % K1) * ITW;
    }
    __syncthreads();                                       // every wave holds its weights: the buffer now takes the conv tile
#pragma unroll 1
    for (int mi = 0; mi < STEM_MT; ++mi) {
        const int m = (wave * STEM_MT + mi) * 32 + r;
        const int mc = m < NP ? m : NP - 1;
        const int ly = mc / CT, lx = mc % CT;
        const _Float16 *xb = xin + 2 * ly * ITW + 2 * lx;
        f32x16 acc[2] = {};
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const uint32_t *xp = reinterpret_cast<const uint32_t *>(xb + xo[c]);
            u32x4 u = {xp[0], xp[1], xp[2], xp[3] & 0xffffu};                // the kx = 7 slot: 0 x 0
            if (c == CHUNKS - 1 && h) u = u32x4{0u, 0u, 0u, 0u};             // the padded row: 0 x 0
            const f16x8 fx = __builtin_bit_cast(f16x8, u);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[c][ct], fx, acc[ct], 0, 0, 0);
        }
        if (m < NP) {
            const bool valid = (unsigned)(cy0 + ly) < (unsigned)Hc && (unsigned)(cx0 + lx) < (unsigned)Wc;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int co = ct * 32 + 8 * j + 4 * h;
                    const float4 b = *reinterpret_cast<const float4 *>(b1 + co);
                    f16x4 v;
                    v[0] = (_Float16)(valid ? fmaxf(acc[ct][4 * j] + b.x, 0.f) : -INFINITY);
                    v[1] = (_Float16)(valid ? fmaxf(acc[ct][4 * j + 1] + b.y, 0.f) : -INFINITY);
                    v[2] = (_Float16)(valid ? fmaxf(acc[ct][4 * j + 2] + b.z, 0.f) : -INFINITY);
                    v[3] = (_Float16)(valid ? fmaxf(acc[ct][4 * j + 3] + b.w, 0.f) : -INFINITY);
                    *reinterpret_cast<f16x4 *>(conv + m * CS + co) = v;
                }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PT * PT * (C1 / 2); i += STEM_THREADS) {
        const int cp = i & (C1 / 2 - 1), p = i >> 5;
        const int ly = p / PT, lx = p % PT, py = py0 + ly, px = px0 + lx;
        if (py >= Hp || px >= Wp) continue;
        float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const f16x2 v = *reinterpret_cast<const f16x2 *>(conv + ((2 * ly + dy) * CT + 2 * lx + dx) * CS + 2 * cp);
                m0 = fmaxf(m0, (float)v[0]);
                m1 = fmaxf(m1, (float)v[1]);
            }
        f16x2 o;
        o[0] = (_Float16)m0;
        o[1] = (_Float16)m1;
        *reinterpret_cast<f16x2 *>(pooled + (((size_t)f * Hp + py) * Wp + px) * C1 + 2 * cp) = o;
    }
}

// ---------------------------------------------------------------------------------------------------
// K_conv2.  k_clip_conv2 on the fp16 core: block = 256 pixels of the frame (four waves of 64) x all 128 channels.
template <bool WLDS>
__global__ void __launch_bounds__(256) k_clip16_conv2(const _Float16 *pooled, const _Float16 *w2, const float *b2, float *partial, int Hp,
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
    if constexpr (WLDS) f16_conv_taps_wlds<C1, 1, MT>(acc, pooled + (size_t)f * P * C1, w2, pt, py, px, pv, 1, Hp, Wp);
    else f16_conv_taps<C1, 1, MT, NT>(acc, pooled + (size_t)f * P * C1, w2, pt, py, px, pv, 1, Hp, Wp);
    f32_tile_sum(acc, b2, m0, P, partial + ((size_t)f * tiles + tile) * C2);
}

// ---------------------------------------------------------------------------------------------------
// K_xproj: clip_xproj (rva_lstm_dev.h) with W_ih1 fp16 in HBM, widened on load.
__global__ void __launch_bounds__(256) k_clip16_xproj(const float *feat_g, const _Float16 *wih1, const float *b1, float *gx, int T, int G4)
{
    clip_xproj(feat_g, wih1, b1, gx, T, G4);
}

// ---------------------------------------------------------------------------------------------------
// K_lstm, launch s: clip_lstm (rva_lstm_dev.h) with W_hh1 and [W_ih2 | W_hh2] fp16 in the slice-major layout of lstm_pack.
__global__ void __launch_bounds__(256) k_clip16_lstm(int s, int T, int hidden, int n_clips, int cap, const _Float16 *whh1,
                                                     const _Float16 *w2, const float *gx, const float *b2, float *h1, float *h2,
                                                     float *c1, float *c2)
{
    clip_lstm(s, T, hidden, n_clips, cap, whh1, w2, gx, b2, h1, h2, c1, c2);
}

// rows x (ka + kb) weights [a | b] -> the slice-major layout of K_lstm, zero-padded
std::vector<_Float16> lstm_pack(const std::vector<_Float16> &a, int ka, const std::vector<_Float16> *b, int kb, int rows)
{
    const int K = ka + kb, KS = lstm_slice(K);
    std::vector<_Float16> out((size_t)rows * LSTM_S * KS, (_Float16)0.f);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < K; ++k)
            out[((size_t)r * LSTM_S + k % LSTM_S) * KS + k / LSTM_S] = k < ka ? a[(size_t)r * ka + k] : (*b)[(size_t)r * kb + k - ka];
    return out;
}

}  // namespace

// The internal entry points of rva_internal.h: the weight rounding of every fp16 plan, and K_stem, shared with rva_resnet_f16.hip.
bool rva_round_f16(const float *src, size_t n, std::vector<_Float16> &dst)
{
    dst.resize(n);
    for (size_t i = 0; i < n; ++i) {
        dst[i] = (_Float16)src[i];
        if (!std::isfinite((float)dst[i])) return false;
    }
    return true;
}

// [co][ci][ky][kx] -> [co][(ci 7 + ky) 8 + kx] in rows of KPS, zero at kx = 7, in row 21 and in the row's tail
std::vector<_Float16> rva_clip16_stem_pack(const std::vector<_Float16> &c1)
{
    std::vector<_Float16> w1((size_t)C1 * KPS, (_Float16)0.f);
    for (int co = 0; co < C1; ++co)
        for (int row = 0; row < 3 * K1; ++row)
            for (int kx = 0; kx < K1; ++kx) w1[(size_t)co * KPS + row * 8 + kx] = c1[((size_t)co * 3 * K1 + row) * K1 + kx];
    return w1;
}

// K_stem keeps its LDS static (51 KB): there is no limit to raise, the call only keeps the shape of rva_clip_stem_prepare
int rva_clip16_stem_prepare(rva_ctx *ctx)
{
    return ctx ? RVA_OK : RVA_ERR_ARG;
}

int rva_clip16_stem_launch(rva_ctx *ctx, const _Float16 *frames, const int32_t *frame_index, const _Float16 *w1, const float *b1,
                           _Float16 *pooled, int H, int W, int n_frames, hipStream_t st)
{
    int Hc, Wc, Hp, Wp;
    rva_stem_maps(H, W, &Hc, &Wc, &Hp, &Wp);
    const int tiles_x = rva_ceil_div(Wp, PT), tiles = tiles_x * rva_ceil_div(Hp, PT);
    k_clip16_stem<<<dim3(tiles, n_frames), STEM_THREADS, 0, st>>>(frames, frame_index, w1, b1, pooled, H, W, Hc, Wc, Hp, Wp, tiles_x);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

// The fp16 plan: the host plan of rva_clip_host.h over this file's kernels.  Every convolution and LSTM weight is rounded once.
struct rva_cnnlstm_f16_plan : rva_cl_plan<_Float16> {
    static constexpr bool REFUSE_LARGE = true;
    static constexpr auto stem_prepare = rva_clip16_stem_prepare;
    static constexpr auto stem = rva_clip16_stem_launch;
    static constexpr auto xproj = k_clip16_xproj;
    static constexpr auto lstm = k_clip16_lstm;
    bool wlds = true;                                // conv2 stages its weights through LDS (A/B switch RVA_CLIP16_WLDS, at creation)

    rva_cnnlstm_f16_plan()
    {
        if (const char *e = getenv("RVA_CLIP16_WLDS")) wlds = atoi(e) != 0;
    }

    // conv1: the stem's packed layout; conv2: [co][ci][ky][kx] -> [co][tap][ci]; W_hh1 and [W_ih2 | W_hh2]: slice-major
    static const char *pack(const rva_cnnlstm_desc &d, const rva_cnnlstm_weights &wt, rva_cl_weights<_Float16> &w)
    {
        const int h = d.hidden, G4 = 4 * h;
        std::vector<_Float16> c1, c2, hh1, ih2, hh2;
        const char *bad = !rva_round_f16(wt.conv1_w, (size_t)C1 * 3 * K1 * K1, c1) ? "conv1_w" :
                          !rva_round_f16(wt.conv2_w, (size_t)C2 * C1 * 9, c2) ? "conv2_w" :
                          !rva_round_f16(wt.w_ih1, (size_t)G4 * C2, w.wih1) ? "w_ih1" : !rva_round_f16(wt.w_hh1, (size_t)G4 * h, hh1) ? "w_hh1" :
                          !rva_round_f16(wt.w_ih2, (size_t)G4 * h, ih2) ? "w_ih2" : !rva_round_f16(wt.w_hh2, (size_t)G4 * h, hh2) ? "w_hh2" : nullptr;
        if (bad) return bad;
        w.w1 = rva_clip16_stem_pack(c1);
        w.w2 = rva_pack_taps_major(c2.data(), C2, C1);
        w.whh1 = lstm_pack(hh1, h, nullptr, 0, G4);
        w.wl2 = lstm_pack(ih2, h, &hh2, h, G4);
        return nullptr;
    }

    void conv2(int nf, hipStream_t st)
    {
        if (wlds) k_clip16_conv2<true><<<dim3(g.conv2_tiles, nf), 256, 0, st>>>(pooled, w2, b2, partial, g.Hp, g.Wp, g.conv2_tiles);
        else k_clip16_conv2<false><<<dim3(g.conv2_tiles, nf), 256, 0, st>>>(pooled, w2, b2, partial, g.Hp, g.Wp, g.conv2_tiles);
    }
};

extern "C" {

int rva_cnnlstm_f16_plan_create(rva_ctx *ctx, const rva_cnnlstm_desc *desc, const rva_cnnlstm_weights *wt, rva_cnnlstm_f16_plan **out)
{
    return rva_cl_create(ctx, "rva_cnnlstm_f16_plan_create", desc, wt, out);
}

void rva_cnnlstm_f16_plan_destroy(rva_cnnlstm_f16_plan *p) { rva_cl_destroy(p); }

int rva_cnnlstm_f16_plan_info(const rva_cnnlstm_f16_plan *p, int32_t *pooled_h, int32_t *pooled_w, int32_t *conv2_tiles, int32_t *n_launches)
{
    return rva_cl_info(p, pooled_h, pooled_w, conv2_tiles, n_launches);
}

int rva_cnnlstm_f16_plan_run(rva_cnnlstm_f16_plan *p, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                             rva_stream_t stream)
{
    return rva_cl_run(p, "rva_cnnlstm_f16_plan_run", frames, frame_index, n_clips, logits, stream);
}

int rva_cnnlstm_f16_plan_run_post(rva_cnnlstm_f16_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                                  void *cls, void *boxes, void *counts, rva_stream_t stream)
{
    return rva_cl_run_post(p, "rva_cnnlstm_f16_plan_run_post", logits, rows, n_rows, max_det, scores, cls, boxes, counts, stream);
}

int rva_cnnlstm_f16_plan_stage(rva_cnnlstm_f16_plan *p, int stage, int n_clips, void *dst, int64_t dst_elems, int64_t *n_elems,
                               rva_stream_t stream)
{
    return rva_cl_stage(p, "rva_cnnlstm_f16_plan_stage", stage, n_clips, dst, dst_elems, n_elems, stream);
}

}  // extern "C"
