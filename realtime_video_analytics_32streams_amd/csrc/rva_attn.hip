// The two fp16 primitives YOLO11 adds to the plan (rva_plan.hip, Builder::build_11): the depthwise 3x3 convolution of the
// detect head's class branch and of the attention block's positional encoding, and the multi-head self-attention of C2PSA over
// the stride-32 map.  Both are entry points of their own (include/rva.h), not rows of the convolution variant table.
//
// rva_dwconv3x3_nhwc_f16 is bandwidth-bound VALU work: a thread owns 8 channels (one 16-byte load per tap) of DW_ROWS vertically
// adjacent outputs, so the three input rows of an output are loaded once and reused by the outputs above and below it (18 loads
// for 4 outputs in place of 36).  Per output: the nine products (exact in fp32) are added from zero in the order (ky, kx), then
// the bias, SiLU (the epilogue's v * rcp(1 + exp(-v))), the residual, and ONE rounding to fp16.
//
// rva_psa_attention_f16 is one kernel from qkv to the heads' outputs: S never leaves registers.  A wave owns 32 queries of one
// (image, head) and walks the keys in tiles of 32 with an online softmax, so any token count is legal and nothing but `tokens`
// fixes the order of a sum.  Per tile:
//   S^T = K Q^T   two v_mfma_f32_32x32x16_f16 (contraction 32); the accumulator has the wave's queries on its lanes and the
//                 tile's 32 keys in its 16 registers x 2 lane halves, so the softmax over keys is a loop over registers plus
//                 one exchange between the halves;
//   p = exp(S^T * 32^-0.5 - m) in fp32 with the running maximum m (keys >= tokens are -inf and never read), the running sum
//                 and the accumulator rescaled by exp(m_old - m);
//   O^T += V^T P^T  P rounded to fp16; the S^T accumulator is the B operand as it stands (its registers 8s .. 8s+7 are k-step s,
//                 k order permuted: element j of half h is key 16s + 8(j>>2) + 4h + (j&3)), and V^T comes from LDS, where the
//                 block's four waves stage the tile transposed ([64 dims][32 keys], 72-byte rows: 4.5 KB).
// At the end O^T is divided by the fp32 row sum and rounded to fp16 once.
#include "rva_internal.h"
#include "rva_mfma_f16.h"

#include <hip/hip_fp16.h>

namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int DW_ROWS = 4;

__device__ __forceinline__ float silu_f(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

__global__ __launch_bounds__(256) void k_dwconv3x3(const _Float16 *__restrict__ in, int ldi, const _Float16 *__restrict__ w,
                                                   const float *__restrict__ bias, _Float16 *__restrict__ out, int ldo,
                                                   const _Float16 *__restrict__ res, int ldr, int B, int H, int W, int C, int act)
{
    const int groups = C / 8, strips = (H + DW_ROWS - 1) / DW_ROWS;
    const long total = (long)B * strips * W * groups;
    long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c0 = (int)(t % groups) * 8; t /= groups;
    const int x = (int)(t % W); t /= W;
    const int y0 = (int)(t % strips) * DW_ROWS, n = (int)(t / strips);
    float wt[9][8], bv[8];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const f16x8 v = *reinterpret_cast<const f16x8 *>(w + (size_t)tap * C + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) wt[tap][j] = (float)v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = bias[c0 + j];
    const _Float16 *img = in + (size_t)n * H * W * ldi + c0;
    auto load = [&](int yy, int xx) -> f16x8 {
        if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) return f16x8{};
        return *reinterpret_cast<const f16x8 *>(img + ((size_t)yy * W + xx) * ldi);
    };
    f16x8 win[3][3];                     // input rows oy - 1, oy, oy + 1 at columns x - 1, x, x + 1
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) { win[1][kx] = load(y0 - 1, x + kx - 1); win[2][kx] = load(y0, x + kx - 1); }
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r) {
        const int oy = y0 + r;
        if (oy >= H) break;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) { win[0][kx] = win[1][kx]; win[1][kx] = win[2][kx]; win[2][kx] = load(oy + 1, x + kx - 1); }
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += (float)win[ky][kx][j] * wt[ky * 3 + kx][j];
        const size_t pix = ((size_t)n * H + oy) * W + x;
        f16x8 rv{};
        if (res) rv = *reinterpret_cast<const f16x8 *>(res + pix * ldr + c0);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = acc[j] + bv[j];
            if (act) v = silu_f(v);
            if (res) v += (float)rv[j];
            o[j] = (_Float16)v;
        }
        *reinterpret_cast<f16x8 *>(out + pix * ldo + c0) = o;
    }
}

constexpr int VT_PITCH = 36;             // fp16 per row of the transposed V tile: 32 keys + 4 (8-byte aligned rows)

__global__ __launch_bounds__(256) void k_psa_attention(const _Float16 *__restrict__ qkv, int ld, _Float16 *__restrict__ out, int ldo, int T)
{
    __shared__ __attribute__((aligned(16))) _Float16 vt[64 * VT_PITCH];
    const int tid = threadIdx.x, wave = tid >> 6, r = tid & 31, h = (tid >> 5) & 1;
    const int head = blockIdx.y, img = blockIdx.z;
    const _Float16 *base = qkv + (size_t)img * T * ld + 128 * head;       // the head's [q 32 | k 32 | v 64] of token 0
    const int q = (blockIdx.x * 4 + wave) * 32 + r;                       // the lane's query (both halves of the wave)
    const bool qv = q < T;
    f16x8 fq[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) fq[s] = qv ? *reinterpret_cast<const f16x8 *>(base + (size_t)q * ld + 16 * s + 8 * h) : f16x8{};
    f32x16 o[2] = {};
    float m = -INFINITY, l = 0.f;
    const float scale = 0.17677669529663687f;                            // 32^-0.5
    for (int k0 = 0; k0 < T; k0 += 32) {
        __syncthreads();                                                  // every wave has read the tile before this one
        {
            const int key = tid >> 3, dc = tid & 7;
            const f16x8 v = k0 + key < T ? *reinterpret_cast<const f16x8 *>(base + (size_t)(k0 + key) * ld + 64 + 8 * dc) : f16x8{};
#pragma unroll
            for (int j = 0; j < 8; ++j) vt[(8 * dc + j) * VT_PITCH + key] = v[j];
        }
        __syncthreads();
        const bool kv = k0 + r < T;
        f32x16 s = {};
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const f16x8 fk = kv ? *reinterpret_cast<const f16x8 *>(base + (size_t)(k0 + r) * ld + 32 + 16 * st + 8 * h) : f16x8{};
            s = __builtin_amdgcn_mfma_f32_32x32x16_f16(fk, fq[st], s, 0, 0, 0);
        }
        float p[16], mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            p[i] = k0 + f32_cd_row(i, h) < T ? s[i] * scale : -INFINITY;
            mt = fmaxf(mt, p[i]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);                                    // finite: key k0 of the tile exists
        const float alpha = __expf(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { p[i] = __expf(p[i] - mn); ps += p[i]; }
        l = l * alpha + ps;
        m = mn;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            f16x8 fp;
#pragma unroll
            for (int j = 0; j < 8; ++j) fp[j] = (_Float16)p[8 * st + j];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const _Float16 *vrow = vt + (32 * dt + r) * VT_PITCH + 16 * st + 4 * h;
                const f16x4 lo = *reinterpret_cast<const f16x4 *>(vrow), hi = *reinterpret_cast<const f16x4 *>(vrow + 8);
                const f16x8 fv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fv, fp, o[dt], 0, 0, 0);
            }
        }
    }
    l += __shfl_xor(l, 32);                                               // the two halves' keys: one fixed order
    if (!qv) return;
    _Float16 *orow = out + ((size_t)img * T + q) * ldo + 64 * head;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (_Float16)(o[dt][4 * g + e] / l);
            *reinterpret_cast<f16x4 *>(orow + 32 * dt + 8 * g + 4 * h) = v;
        }
}

}  // namespace

extern "C" {

int rva_dwconv3x3_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias, void *out, int ldo,
                           const void *residual, int ldr, int batch, int H, int W, int C, int act, rva_stream_t stream)
{
    if (!ctx) return RVA_ERR_ARG;
    if (!in || !weights || !bias || !out || batch <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || ldi < C || ldo < C || ldi % 8 || ldo % 8 ||
        (residual && (ldr < C || ldr % 8)) || ((uintptr_t)in | (uintptr_t)out | (uintptr_t)weights | (uintptr_t)residual) % 16 ||
        (uintptr_t)bias % 4)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_dwconv3x3_nhwc_f16: batch, H, W > 0, C %% 8 == 0, ldi / ldo / ldr >= C and multiples of 8, 16-byte pointers");
    const long threads = (long)batch * ((H + DW_ROWS - 1) / DW_ROWS) * W * (C / 8);
    if ((threads + 255) / 256 > 0x7fffffffL) return rva_fail(ctx, RVA_ERR_ARG, "rva_dwconv3x3_nhwc_f16: too many outputs for one launch");
    k_dwconv3x3<<<(unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>((const _Float16 *)in, ldi, (const _Float16 *)weights, bias,
                                                                                  (_Float16 *)out, ldo, (const _Float16 *)residual, ldr, batch, H, W,
                                                                                  C, act ? 1 : 0);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

int rva_psa_attention_f16(rva_ctx *ctx, const void *qkv, int ld, void *out, int ldo, int batch, int tokens, int heads, rva_stream_t stream)
{
    if (!ctx) return RVA_ERR_ARG;
    if (!qkv || !out || batch < 1 || batch > 65535 || tokens < 1 || heads < 1 || heads > 65535 || ld < 128 * heads || ldo < 64 * heads || ld % 8 ||
        ldo % 8 || ((uintptr_t)qkv | (uintptr_t)out) % 16)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_psa_attention_f16: batch, tokens, heads >= 1, ld >= 128 heads, ldo >= 64 heads, ld and ldo multiples of 8, 16-byte pointers");
    const dim3 grid((unsigned)((tokens + 127) / 128), (unsigned)heads, (unsigned)batch);
    k_psa_attention<<<grid, 256, 0, (hipStream_t)stream>>>((const _Float16 *)qkv, ld, (_Float16 *)out, ldo, tokens);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

}  // extern "C"
