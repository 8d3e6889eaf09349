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
//   K_xproj  as k_clip_xproj with W_ih1 fp16 in HBM (a thread's row is 16 contiguous 16-byte reads), widened on load; fmaf chain
//            over k = 0..127 in order, + b1.
//   K_lstm   the T + 1 diagonal launches of k_clip_lstm with W_hh1 and [W_ih2 | W_hh2] fp16 in HBM, widened on load.  Thread
//            (gate row, k-slice sigma) owns k = sigma, sigma + 16, ...: the weights are stored slice-major, [row][sigma][j] =
//            W[row][sigma + 16 j], each slice zero-padded to a multiple of 8, so a lane reads contiguous 16 bytes.  Gate
//            pre-activation = base + the 16 slice sums in order, each an fmaf chain from zero over j in order (a padded j adds
//            0 x 0); gate formulas, h and c are k_clip_lstm's, fp32.
//   K_mean / K_head / K_post: the kernels of rva_clip.hip.
#include "rva_internal.h"
#include "rva_mfma_f16.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int C1 = 64, C2 = 128, K1 = 7;                  // stem widths of the architecture
constexpr int PT = 8;                                      // pooled tile (PT x PT) of K_stem
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
constexpr int LSTM_U = 4, LSTM_S = 16, LSTM_G = 8;         // units per block, k-slices, clips per pass
constexpr int LSTM_R = 4 * LSTM_U;                         // gate rows per block
constexpr int MAX_HIDDEN = 1024, MAX_T = 64, MAX_CLASSES = RVA_PLAN_MAX_CLASSES;

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
// K_xproj.  Block = (256 gate rows, one clip): gx[clip][t][row] = (sum_k W_ih1[row][k] * feat[t][k], k = 0..127 in order) + b1[row].
__global__ void __launch_bounds__(256) k_clip16_xproj(const float *feat_g, const _Float16 *wih1, const float *b1, float *gx, int T, int G4)
{
    extern __shared__ float feat[];                        // [T][C2]
    const int clip = blockIdx.y;
    for (int i = threadIdx.x; i < T * C2; i += 256) feat[i] = feat_g[(size_t)clip * T * C2 + i];
    __syncthreads();
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= G4) return;
    float w[C2];
    const f16x8 *wr = reinterpret_cast<const f16x8 *>(wih1 + (size_t)row * C2);
#pragma unroll
    for (int q = 0; q < C2 / 8; ++q) {
        const f16x8 v = wr[q];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[8 * q + e] = (float)v[e];
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

// slice length of a K-wide LSTM operand: ceil(K / 16) rounded up to whole 16-byte loads
__host__ __device__ inline int lstm_slice(int K) { return (((K + LSTM_S - 1) / LSTM_S) + 7) & ~7; }

// ---------------------------------------------------------------------------------------------------
// K_lstm, launch s: k_clip_lstm (rva_clip.hip) with fp16 weights in the slice-major layout.  blockIdx.y = 0 -> layer 1 at step s
// (s < T), blockIdx.y = 1 -> layer 2 at step s-1 (s >= 1).  Block = units [u0, u0+4) x four gates (16 rows) x every clip, eight
// clips per pass.  Layer 1: x = h1[s-1] (zero at s = 0), K = h, base = gx[clip][s][row].  Layer 2: x = [h1[s-1], h2[s-2]], K = 2h,
// base = b2[row].  xs holds x per clip zero-padded to 16 slices of lstm_slice(K): xs[g][16 j + sigma] = x[sigma + 16 j].
__global__ void __launch_bounds__(256) k_clip16_lstm(int s, int T, int hidden, int n_clips, int cap, const _Float16 *whh1,
                                                     const _Float16 *w2, const float *gx, const float *b2, float *h1, float *h2,
                                                     float *c1, float *c2)
{
    extern __shared__ float lds[];
    const int layer = blockIdx.y;
    if ((layer == 0 && s >= T) || (layer == 1 && s == 0)) return;
    const int step = layer == 0 ? s : s - 1;
    const int K = layer == 0 ? hidden : 2 * hidden;
    const int KS = lstm_slice(K), KPAD = LSTM_S * KS;
    const int G4 = 4 * hidden;
    float *xs = lds;                                       // [LSTM_G][KPAD]
    float *part = xs + LSTM_G * LSTM_S * lstm_slice(2 * hidden);   // [LSTM_R][LSTM_S][LSTM_G]
    float *gates = part + LSTM_R * LSTM_S * LSTM_G;        // [LSTM_R][LSTM_G]
    const int u0 = blockIdx.x * LSTM_U;
    const int rho = threadIdx.x / LSTM_S, sig = threadIdx.x % LSTM_S;
    const int ju = rho % LSTM_U, gate = rho / LSTM_U;
    const bool rv = u0 + ju < hidden;
    const int grow = gate * hidden + (rv ? u0 + ju : 0);
    const _Float16 *Wr = (layer == 0 ? whh1 : w2) + ((size_t)grow * LSTM_S + sig) * KS;
    const float *hprev1 = step >= 1 || layer == 1 ? h1 + (size_t)(layer == 0 ? step - 1 : step) * cap * hidden : nullptr;
    const float *hprev2 = layer == 1 && step >= 1 ? h2 + (size_t)(step - 1) * cap * hidden : nullptr;
    float *cst = layer == 0 ? c1 : c2;
    float *hout = (layer == 0 ? h1 : h2) + (size_t)step * cap * hidden;
    // the weight loads run two ahead of their use, and the first two are issued before the fill of xs (they do not depend on x):
    // the HBM latency of a thread's slice runs beside the fill
    auto ldw = [&](int j0) { return j0 < KS ? *reinterpret_cast<const f16x8 *>(Wr + j0) : f16x8{}; };
    for (int b0 = 0; b0 < n_clips; b0 += LSTM_G) {
        f16x8 wa = ldw(0), wb = ldw(8);
        __syncthreads();
        for (int i0 = threadIdx.x; i0 < LSTM_G * KPAD; i0 += 256 * 8) {        // eight loads in flight, then eight LDS stores
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = i0 + 256 * j;
                const int g = i / KPAD, k = i % KPAD, b = b0 + g;
                v[j] = 0.f;
                if (i < LSTM_G * KPAD && b < n_clips && k < K) {
                    if (k < hidden) v[j] = hprev1 ? hprev1[(size_t)b * hidden + k] : 0.f;
                    else v[j] = hprev2 ? hprev2[(size_t)b * hidden + k - hidden] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (i0 + 256 * j < LSTM_G * KPAD) xs[i0 + 256 * j] = v[j];
        }
        __syncthreads();
        float acc[LSTM_G];
#pragma unroll
        for (int g = 0; g < LSTM_G; ++g) acc[g] = 0.f;
        for (int j0 = 0; j0 < KS; j0 += 8) {
            const f16x8 wv = wa;
            wa = wb;
            wb = ldw(j0 + 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float wf = (float)wv[e];
                const float *xk = xs + (j0 + e) * LSTM_S + sig;
#pragma unroll
                for (int g = 0; g < LSTM_G; ++g) acc[g] = fmaf(wf, xk[g * KPAD], acc[g]);
            }
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

size_t lstm_lds(int hidden)
{
    return (size_t)(LSTM_G * LSTM_S * lstm_slice(2 * hidden) + LSTM_R * LSTM_S * LSTM_G + LSTM_R * LSTM_G) * sizeof(float);
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

struct rva_cnnlstm_f16_plan {
    rva_ctx *ctx = nullptr;
    rva_cnnlstm_desc d{};
    int Hc = 0, Wc = 0, Hp = 0, Wp = 0, conv2_tiles = 0;
    _Float16 *w1 = nullptr, *w2 = nullptr, *wih1 = nullptr, *whh1 = nullptr, *wl2 = nullptr, *pooled = nullptr;
    float *b1 = nullptr, *b2 = nullptr, *bl1 = nullptr, *bl2 = nullptr, *wh = nullptr, *bh = nullptr;
    float *partial = nullptr, *feat = nullptr, *gx = nullptr, *h1 = nullptr, *h2 = nullptr, *c1 = nullptr, *c2 = nullptr;
    bool wlds = true;                                // conv2 stages its weights through LDS (A/B switch RVA_CLIP16_WLDS)
    rva_dev_arena mem;
};

extern "C" {

int rva_cnnlstm_f16_plan_create(rva_ctx *ctx, const rva_cnnlstm_desc *desc, const rva_cnnlstm_weights *wt, rva_cnnlstm_f16_plan **out)
{
    if (!ctx || !desc || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_f16_plan_create: null argument");
    *out = nullptr;
    const rva_cnnlstm_desc d = *desc;
    if (d.height < 2 || d.width < 2 || d.frames < 1 || d.frames > MAX_T || d.hidden < 1 || d.hidden > MAX_HIDDEN || d.classes < 1 ||
        d.classes > MAX_CLASSES || d.max_clips < 1 || (int64_t)d.max_clips * d.frames > 65535 || (int64_t)d.height * d.width > (1 << 26))
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_f16_plan_create: bad descriptor (frames 1..%d, hidden 1..%d, classes 1..%d, "
                        "max_clips >= 1, max_clips * frames <= 65535)", MAX_T, MAX_HIDDEN, MAX_CLASSES);
    if (!wt->conv1_w || !wt->conv1_b || !wt->conv2_w || !wt->conv2_b || !wt->w_ih1 || !wt->b1 || !wt->w_hh1 || !wt->w_ih2 ||
        !wt->w_hh2 || !wt->b2 || !wt->head_w || !wt->head_b)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_f16_plan_create: every weight array is required");
    const int h = d.hidden, G4 = 4 * h, T = d.frames;
    std::vector<_Float16> c1, c2, ih1, hh1, ih2, hh2;
    const char *bad = !rva_round_f16(wt->conv1_w, (size_t)C1 * 3 * K1 * K1, c1) ? "conv1_w" :
                      !rva_round_f16(wt->conv2_w, (size_t)C2 * C1 * 9, c2) ? "conv2_w" :
                      !rva_round_f16(wt->w_ih1, (size_t)G4 * C2, ih1) ? "w_ih1" : !rva_round_f16(wt->w_hh1, (size_t)G4 * h, hh1) ? "w_hh1" :
                      !rva_round_f16(wt->w_ih2, (size_t)G4 * h, ih2) ? "w_ih2" : !rva_round_f16(wt->w_hh2, (size_t)G4 * h, hh2) ? "w_hh2" : nullptr;
    if (bad) return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_f16_plan_create: a value of %s does not stay finite in fp16", bad);
    // conv1: the stem's packed layout; conv2: [co][ci][ky][kx] -> [co][tap][ci]
    const std::vector<_Float16> w1 = rva_clip16_stem_pack(c1), w2 = rva_pack_taps_major(c2.data(), C2, C1);
    const std::vector<_Float16> whh1 = lstm_pack(hh1, h, nullptr, 0, G4), wl2 = lstm_pack(ih2, h, &hh2, h, G4);
    auto *p = new rva_cnnlstm_f16_plan();
    p->ctx = ctx;
    p->d = d;
    if (const char *e = getenv("RVA_CLIP16_WLDS")) p->wlds = atoi(e) != 0;
    rva_stem_maps(d.height, d.width, &p->Hc, &p->Wc, &p->Hp, &p->Wp);
    p->conv2_tiles = rva_ceil_div(p->Hp * p->Wp, 256);
    const size_t nf = (size_t)d.max_clips * T, mc = (size_t)d.max_clips;
    const size_t n_pooled = nf * p->Hp * p->Wp * C1, n_part = nf * p->conv2_tiles * C2;
    const size_t need = (n_pooled + w1.size() + w2.size() + ih1.size() + whh1.size() + wl2.size()) * sizeof(_Float16) +
                        (n_part + nf * C2 + nf * G4 + 2 * (size_t)T * mc * h + 2 * mc * h + C1 + C2 + 2 * (size_t)G4 +
                         (size_t)d.classes * (h + 1)) * sizeof(float);
    char shape[64];
    snprintf(shape, sizeof shape, "%d clips of %d x %d x %d", d.max_clips, T, d.height, d.width);
    int rc = rva_plan_fits(ctx, "rva_cnnlstm_f16_plan_create", need, shape);
    if (rc != RVA_OK) {
        delete p;
        return rc;
    }
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    step(p->mem.upload(ctx, &p->w1, w1.data(), w1.size()));
    step(p->mem.upload(ctx, &p->b1, wt->conv1_b, C1));
    step(p->mem.upload(ctx, &p->w2, w2.data(), w2.size()));
    step(p->mem.upload(ctx, &p->b2, wt->conv2_b, C2));
    step(p->mem.upload(ctx, &p->wih1, ih1.data(), ih1.size()));
    step(p->mem.upload(ctx, &p->bl1, wt->b1, G4));
    step(p->mem.upload(ctx, &p->whh1, whh1.data(), whh1.size()));
    step(p->mem.upload(ctx, &p->wl2, wl2.data(), wl2.size()));
    step(p->mem.upload(ctx, &p->bl2, wt->b2, G4));
    step(p->mem.upload(ctx, &p->wh, wt->head_w, (size_t)d.classes * h));
    step(p->mem.upload(ctx, &p->bh, wt->head_b, d.classes));
    step(p->mem.alloc(ctx, &p->pooled, n_pooled));
    step(p->mem.alloc(ctx, &p->partial, n_part));
    step(p->mem.alloc(ctx, &p->feat, nf * C2));
    step(p->mem.alloc(ctx, &p->gx, nf * G4));
    step(p->mem.alloc(ctx, &p->h1, (size_t)T * mc * h));
    step(p->mem.alloc(ctx, &p->h2, (size_t)T * mc * h));
    step(p->mem.alloc(ctx, &p->c1, mc * h));
    step(p->mem.alloc(ctx, &p->c2, mc * h));
    if (rc == RVA_OK && rva_func_smem((const void *)k_clip16_lstm, lstm_lds(h)) != hipSuccess)
        rc = rva_fail(ctx, RVA_ERR_HIP, "rva_cnnlstm_f16_plan_create: cannot raise the LSTM kernel's LDS limit");
    if (rc == RVA_OK) rc = rva_clip16_stem_prepare(ctx);
    if (rc == RVA_OK) rc = rva_clip_head_prepare(ctx, h);
    if (rc == RVA_OK) rc = rva_clip_post_prepare(ctx, d.classes);
    if (rc != RVA_OK) {
        rva_cnnlstm_f16_plan_destroy(p);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

void rva_cnnlstm_f16_plan_destroy(rva_cnnlstm_f16_plan *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

int rva_cnnlstm_f16_plan_info(const rva_cnnlstm_f16_plan *p, int32_t *pooled_h, int32_t *pooled_w, int32_t *conv2_tiles, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    if (pooled_h) *pooled_h = p->Hp;
    if (pooled_w) *pooled_w = p->Wp;
    if (conv2_tiles) *conv2_tiles = p->conv2_tiles;
    if (n_launches) *n_launches = 4 + (p->d.frames + 1) + 1;
    return RVA_OK;
}

int rva_cnnlstm_f16_plan_run(rva_cnnlstm_f16_plan *p, const void *frames, const int32_t *frame_index, int n_clips, void *logits,
                             rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_f16_plan_run: bad argument (n_clips %d, capacity %d)", n_clips, p->d.max_clips);
    const hipStream_t st = (hipStream_t)stream_;
    const int T = p->d.frames, h = p->d.hidden, G4 = 4 * h, nf = n_clips * T;
    int rc = rva_clip16_stem_launch(ctx, (const _Float16 *)frames, frame_index, p->w1, p->b1, p->pooled, p->d.height, p->d.width, nf, st);
    if (rc != RVA_OK) return rc;
    if (p->wlds) k_clip16_conv2<true><<<dim3(p->conv2_tiles, nf), 256, 0, st>>>(p->pooled, p->w2, p->b2, p->partial, p->Hp, p->Wp, p->conv2_tiles);
    else k_clip16_conv2<false><<<dim3(p->conv2_tiles, nf), 256, 0, st>>>(p->pooled, p->w2, p->b2, p->partial, p->Hp, p->Wp, p->conv2_tiles);
    RVA_HIP(ctx, hipGetLastError());
    rc = rva_clip_mean_launch(ctx, p->partial, p->conv2_tiles, (float)(p->Hp * p->Wp), p->feat, nf, C2, st);
    if (rc != RVA_OK) return rc;
    k_clip16_xproj<<<dim3(rva_ceil_div(G4, 256), n_clips), 256, (size_t)T * C2 * sizeof(float), st>>>(p->feat, p->wih1, p->bl1, p->gx, T, G4);
    RVA_HIP(ctx, hipGetLastError());
    for (int s = 0; s <= T; ++s) {
        k_clip16_lstm<<<dim3(rva_ceil_div(h, LSTM_U), 2), 256, lstm_lds(h), st>>>(s, T, h, n_clips, p->d.max_clips, p->whh1, p->wl2,
                                                                                  p->gx, p->bl2, p->h1, p->h2, p->c1, p->c2);
        RVA_HIP(ctx, hipGetLastError());
    }
    return rva_clip_head_launch(ctx, p->h2 + (size_t)(T - 1) * p->d.max_clips * h, p->wh, p->bh, (float *)logits, h, p->d.classes,
                                n_clips, st);
}

int rva_cnnlstm_f16_plan_run_post(rva_cnnlstm_f16_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                                  void *cls, void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, "rva_cnnlstm_f16_plan_run_post", (const float *)logits, p->d.classes, std::min(5, p->d.classes), rows,
                                n_rows, max_det, (float *)scores, (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  POOLED is fp16 elements, every other
// stage fp32, and the counts are element counts; h1 / h2 of fewer clips than the capacity are T rows of n_clips * hidden out of a
// pitch of max_clips * hidden: one 2D copy.
int rva_cnnlstm_f16_plan_stage(rva_cnnlstm_f16_plan *p, int stage, int n_clips, void *dst, int64_t dst_elems, int64_t *n_elems,
                               rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_f16_plan_stage: bad argument (n_clips %d, capacity %d)", n_clips, p->d.max_clips);
    const int64_t T = p->d.frames, h = p->d.hidden, nf = (int64_t)n_clips * T;
    const void *src = nullptr;
    int64_t count = 0;
    switch (stage) {
    case RVA_CNNLSTM_STAGE_POOLED: src = p->pooled; count = nf * p->Hp * p->Wp * C1; break;
    case RVA_CNNLSTM_STAGE_PARTIAL: src = p->partial; count = nf * p->conv2_tiles * C2; break;
    case RVA_CNNLSTM_STAGE_FEAT: src = p->feat; count = nf * C2; break;
    case RVA_CNNLSTM_STAGE_GX: src = p->gx; count = nf * 4 * h; break;
    case RVA_CNNLSTM_STAGE_H1: src = p->h1; count = nf * h; break;
    case RVA_CNNLSTM_STAGE_H2: src = p->h2; count = nf * h; break;
    default: return rva_fail(ctx, RVA_ERR_ARG, "rva_cnnlstm_f16_plan_stage: unknown stage %d", stage);
    }
    const bool rows = (stage == RVA_CNNLSTM_STAGE_H1 || stage == RVA_CNNLSTM_STAGE_H2) && n_clips < p->d.max_clips;
    const bool f16 = stage == RVA_CNNLSTM_STAGE_POOLED;    // the size error of an fp32 stage says "floats", as the fp32 plan's
    return rva_clip_stage_copy(ctx, "rva_cnnlstm_f16_plan_stage", stage, n_clips, "clips", src, f16 ? sizeof(_Float16) : sizeof(float),
                               f16 ? "elements" : "floats", count, rows ? T : 0, n_clips * h, p->d.max_clips * h, dst, dst_elems, n_elems,
                               (hipStream_t)stream_);
}

}  // extern "C"
