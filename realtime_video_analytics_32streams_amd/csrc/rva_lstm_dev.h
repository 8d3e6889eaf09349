// The bodies of K_xproj and K_lstm of the CNN-LSTM plans, written once over the weight element WE (float: rva_clip.hip, _Float16:
// rva_clip_f16.hip); each file's __global__ kernel is a one-line caller.  The two precisions differ for real only in how a thread
// gets its weights -- row-major fp32 against slice-major fp16 with a two-ahead prefetch -- and in how x lies in LDS for that: an
// overload in K_xproj, one `if constexpr` arm each in K_lstm.  A body is one function, not pieces called from two kernels: the
// compiler simplifies a callee before it inlines it, and pieces changed both kernels' registers and size; whole, they stay as
// they were (profiles/clip_one_plan.json).
#pragma once

#include <type_traits>

#include "rva_mfma_f16.h"
#include "rva_plan_topo.h"

constexpr int LSTM_U = 4, LSTM_S = 16, LSTM_G = 8;         // units per block, k-slices, clips per pass
constexpr int LSTM_R = 4 * LSTM_U;                         // gate rows per block

// ---------------------------------------------------------------------------------------------------
// K_xproj.  Block = (256 gate rows, one clip): gx[clip][t][row] = (sum_k W_ih1[row][k] * feat[t][k], k = 0..127 in order) + b1[row].
// A thread keeps its weight row in fp32 registers: 32 float4 reads, or 16 reads of eight fp16 widened on load.
__device__ __forceinline__ void xproj_row(float (&w)[CL_C2], const float *row)
{
    const float4 *wr = reinterpret_cast<const float4 *>(row);
#pragma unroll
    for (int q = 0; q < CL_C2 / 4; ++q) {
        const float4 v = wr[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
}

__device__ __forceinline__ void xproj_row(float (&w)[CL_C2], const _Float16 *row)
{
    const f16x8 *wr = reinterpret_cast<const f16x8 *>(row);
#pragma unroll
    for (int q = 0; q < CL_C2 / 8; ++q) {
        const f16x8 v = wr[q];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[8 * q + e] = (float)v[e];
    }
}

template <class WE>
__device__ __forceinline__ void clip_xproj(const float *feat_g, const WE *wih1, const float *b1, float *gx, int T, int G4)
{
    extern __shared__ float feat[];                        // [T][C2]
    const int clip = blockIdx.y;
    for (int i = threadIdx.x; i < T * CL_C2; i += 256) feat[i] = feat_g[(size_t)clip * T * CL_C2 + i];
    __syncthreads();
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= G4) return;
    float w[CL_C2];
    xproj_row(w, wih1 + (size_t)row * CL_C2);
    const float b = b1[row];
    for (int t = 0; t < T; ++t) {
        const float *x = feat + t * CL_C2;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < CL_C2; ++k) s = fmaf(w[k], x[k], s);
        gx[((size_t)clip * T + t) * G4 + row] = s + b;
    }
}

// ---------------------------------------------------------------------------------------------------
// K_lstm, launch s: blockIdx.y = 0 -> layer 1 at step s (s < T), blockIdx.y = 1 -> layer 2 at step s-1 (s >= 1).  Block = units
// [u0, u0+4) x all four gates (16 rows) x every clip, eight clips per pass; thread = (gate row rho, k-slice sigma), which owns k =
// sigma, sigma+16, ...  Layer 1: x = h1[s-1] (zero at s = 0), K = hidden, W = W_hh1 [4h][h], base = gx[clip][s][row].  Layer 2: x =
// [h1[s-1], h2[s-2]] (h2 zero at step 0), K = 2 hidden, W = [W_ih2 | W_hh2] [4h][2h], base = b2[row].  Gate pre-activation = base +
// the 16 slice sums in order, each an fmaf chain from zero over the slice's k in order.  Cell: sigmoid(x) = 1 / (1 + expf(-x)),
// tanh(x) = 1 - 2 / (expf(2x) + 1); c = f*c + i*g, h = o*tanh(c) (c = 0 at step 0).  h1 / h2 are [T][cap][hidden]: launch s writes
// h1[s] and h2[s-1], and reads only h1[s-1] and h2[s-2].
//
// The schedule, the block's share, the gate sums and the cell are written once.  How a thread gets its weights, and with it how
// x lies in LDS, differs for real and is one arm each:
//   WE = float     W row-major in HBM; xs = x of eight clips, [LSTM_G][K]; a thread reads its slice element by element.
//   WE = _Float16  W slice-major, [row][sigma][j] = W[row][sigma + 16 j], each slice zero-padded to lstm_slice(K) (whole 16-byte
//                  loads), widened on load; xs[g][16 j + sigma] = x[sigma + 16 j], zero-padded alike (a padded j adds 0 x 0).
//                  The weight loads run two ahead of their use, and the first two are issued before the fill of xs (they do not
//                  depend on x): the HBM latency of a thread's slice runs beside the fill.

// slice length of a K-wide fp16 LSTM operand: ceil(K / 16) rounded up to whole 16-byte loads
__host__ __device__ inline int lstm_slice(int K) { return (((K + LSTM_S - 1) / LSTM_S) + 7) & ~7; }

// dynamic LDS of a K_lstm block: xs at its widest (layer 2), part, gates
template <class WE>
size_t lstm_lds(int hidden)
{
    const int xs = std::is_same<WE, float>::value ? LSTM_G * 2 * hidden : LSTM_G * LSTM_S * lstm_slice(2 * hidden);
    return (size_t)(xs + LSTM_R * LSTM_S * LSTM_G + LSTM_R * LSTM_G) * sizeof(float);
}

template <class WE>
__device__ __forceinline__ void clip_lstm(int s, int T, int hidden, int n_clips, int cap, const WE *whh1, const WE *w2, const float *gx,
                                          const float *b2, float *h1, float *h2, float *c1, float *c2)
{
    constexpr bool SLICED = !std::is_same<WE, float>::value;
    extern __shared__ float lds[];
    const int layer = blockIdx.y;
    if ((layer == 0 && s >= T) || (layer == 1 && s == 0)) return;
    const int step = layer == 0 ? s : s - 1;
    const int K = layer == 0 ? hidden : 2 * hidden;
    const int KS = lstm_slice(K), KPAD = LSTM_S * KS;      // SLICED only
    const int G4 = 4 * hidden;
    float *xs = lds;                                       // [LSTM_G][K], SLICED: [LSTM_G][KPAD]
    float *part = xs + (SLICED ? LSTM_G * LSTM_S * lstm_slice(2 * hidden) : LSTM_G * K);   // [LSTM_R][LSTM_S][LSTM_G]
    float *gates = part + LSTM_R * LSTM_S * LSTM_G;        // [LSTM_R][LSTM_G]
    const int u0 = blockIdx.x * LSTM_U;
    const int rho = threadIdx.x / LSTM_S, sig = threadIdx.x % LSTM_S;
    const int ju = rho % LSTM_U, gate = rho / LSTM_U;
    const bool rv = u0 + ju < hidden;
    const int grow = gate * hidden + (rv ? u0 + ju : 0);
    const WE *W = (layer == 0 ? whh1 : w2) + (SLICED ? ((size_t)grow * LSTM_S + sig) * KS : (size_t)grow * K);
    const float *hprev1 = step >= 1 || layer == 1 ? h1 + (size_t)(layer == 0 ? step - 1 : step) * cap * hidden : nullptr;
    const float *hprev2 = layer == 1 && step >= 1 ? h2 + (size_t)(step - 1) * cap * hidden : nullptr;
    float *cst = layer == 0 ? c1 : c2;
    float *hout = (layer == 0 ? h1 : h2) + (size_t)step * cap * hidden;
    for (int b0 = 0; b0 < n_clips; b0 += LSTM_G) {
        float acc[LSTM_G];
        if constexpr (SLICED) {
            auto ldw = [&](int j0) { return j0 < KS ? *reinterpret_cast<const f16x8 *>(W + j0) : f16x8{}; };
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
        } else {
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
#pragma unroll
            for (int g = 0; g < LSTM_G; ++g) acc[g] = 0.f;
            for (int k = sig; k < K; k += LSTM_S) {
                const float wv = W[k];
#pragma unroll
                for (int g = 0; g < LSTM_G; ++g) acc[g] = fmaf(wv, xs[g * K + k], acc[g]);
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
