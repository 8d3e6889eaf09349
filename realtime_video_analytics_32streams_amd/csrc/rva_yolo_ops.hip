// The detectors' kernels that are not convolutions (NHWC fp16), each beside its entry point: SPPF's chained max pools, the 5x5
// max pool, the FPN's nearest 2x upsample and the detect head's decode (DFL + dist2bbox + sigmoid).  store_scores8, which the
// decoding epilogue of k_conv_gbig<..., HEAD> (rva_conv.hip) shares with head_anchor, is in rva_conv_dev.h.
#include "rva_conv_dev.h"

namespace {

// 5x5 stride-1 pad-2 max pool over a channel slice (C % 8 == 0): thread = (pixel, 8 channels)
__global__ void __launch_bounds__(256) k_maxpool5(const __half *in, int ldi, __half *out, int ldo, int B, int H, int W, int C)
{
    const int cg = C >> 3;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * H * W * cg) return;
    const int g = (int)(idx % cg);
    const long pix = idx / cg;
    const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
    h8 mx;
#pragma unroll
    for (int t = 0; t < 8; ++t) mx[t] = (_Float16)-65504.f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy;
        if ((unsigned)yy >= (unsigned)H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx;
            if ((unsigned)xx >= (unsigned)W) continue;
            const h8 v = *reinterpret_cast<const h8 *>(in + ((size_t)(b * H + yy) * W + xx) * ldi + g * 8);
            mx = __builtin_elementwise_max(mx, v);
        }
    }
    *reinterpret_cast<h8 *>(out + (size_t)pix * ldo + g * 8) = mx;
}

// nearest 2x upsample: out pixel (y, x) <- in pixel (y/2, x/2); thread = (out pixel, 8 channels)
__global__ void __launch_bounds__(256) k_upsample2(const __half *in, int ldi, __half *out, int ldo, int B, int H, int W, int C)
{
    const int cg = C >> 3, Ho = H * 2, Wo = W * 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * Ho * Wo * cg) return;
    const int g = (int)(idx % cg);
    const long pix = idx / cg;
    const int x = (int)(pix % Wo), y = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
    const uint4 v = *reinterpret_cast<const uint4 *>(in + ((size_t)(b * H + (y >> 1)) * W + (x >> 1)) * ldi + g * 8);
    *reinterpret_cast<uint4 *>(out + (size_t)pix * ldo + g * 8) = v;
}

}  // namespace

extern "C" int rva_upsample2x_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, void *out, int ldo, int batch, int H, int W, int C,
                                       rva_stream_t stream_)
{
    if (!ctx || !in || !out || C % 8 || ldi % 8 || ldo % 8) return rva_fail(ctx, RVA_ERR_ARG, "rva_upsample2x_nhwc_f16: bad argument");
    const long n = (long)batch * H * 2 * W * 2 * (C / 8);
    k_upsample2<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>((const __half *)in, ldi, (__half *)out, ldo, batch, H, W, C);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

extern "C" int rva_maxpool5_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, void *out, int ldo, int batch, int H, int W, int C,
                                     rva_stream_t stream_)
{
    if (!ctx || !in || !out || C % 8 || ldi % 8 || ldo % 8) return rva_fail(ctx, RVA_ERR_ARG, "rva_maxpool5_nhwc_f16: bad argument");
    const long n = (long)batch * H * W * (C / 8);
    k_maxpool5<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>((const __half *)in, ldi, (__half *)out, ldo, batch, H, W, C);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------------
// The three chained 5x5 max pools of SPPF in one launch.  pool5(pool5(x)) = pool9(x) and pool5^3(x) = pool13(x)
// (stride 1, -inf padding: the windows just grow), so all three outputs are separable running maxima of the same tile:
// a block holds one image x 8 channels in LDS, does the row pass for window radii 2 / 4 / 6, then the column pass,
// and writes y1, y2, y3 into their channel slices.  Replaces three dependent launches that each re-read 25 taps from L2.
__global__ void __launch_bounds__(256) k_sppf_pool3(const __half *in, int ldi, __half *o1, __half *o2, __half *o3, int ldo,
                                                    int H, int W, int C)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int HW = H * W, cg = C >> 3;
    h8 *x = (h8 *)smem;                  // [HW]
    h8 *r5 = x + HW, *r9 = r5 + HW, *r13 = r9 + HW;
    const int b = blockIdx.x / cg, g = blockIdx.x - b * cg;
    const size_t base = (size_t)b * HW;
    for (int p = threadIdx.x; p < HW; p += 256) x[p] = *reinterpret_cast<const h8 *>(in + (base + p) * ldi + g * 8);
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += 256) {
        const int y = p / W, xx = p - y * W;
        h8 m = x[p];
#pragma unroll
        for (int d = 1; d <= 6; ++d) {
            if (xx - d >= 0) m = __builtin_elementwise_max(m, x[p - d]);
            if (xx + d < W) m = __builtin_elementwise_max(m, x[p + d]);
            if (d == 2) r5[p] = m;
            if (d == 4) r9[p] = m;
        }
        r13[p] = m;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += 256) {
        const int y = p / W;
        h8 m5 = r5[p], m9 = r9[p], m13 = r13[p];
#pragma unroll
        for (int d = 1; d <= 6; ++d) {
            if (y - d >= 0) {
                if (d <= 2) m5 = __builtin_elementwise_max(m5, r5[p - d * W]);
                if (d <= 4) m9 = __builtin_elementwise_max(m9, r9[p - d * W]);
                m13 = __builtin_elementwise_max(m13, r13[p - d * W]);
            }
            if (y + d < H) {
                if (d <= 2) m5 = __builtin_elementwise_max(m5, r5[p + d * W]);
                if (d <= 4) m9 = __builtin_elementwise_max(m9, r9[p + d * W]);
                m13 = __builtin_elementwise_max(m13, r13[p + d * W]);
            }
        }
        const size_t o = (base + p) * ldo + g * 8;
        *reinterpret_cast<h8 *>(o1 + o) = m5;
        *reinterpret_cast<h8 *>(o2 + o) = m9;
        *reinterpret_cast<h8 *>(o3 + o) = m13;
    }
}

// The same with G groups of 8 channels per block (round 4): consecutive lanes take the G 16-byte pieces of one pixel and then the
// next pixel, so a wave touches whole 64-byte (G = 4) runs of the NHWC rows instead of one 16-byte piece per 512-byte row, for the
// loads and for the three stores alike.  1024 threads; the 13-wide row maxima replace the input tile in LDS (they are held in
// registers across a barrier), so a block needs 3 x HW x G x 16 bytes.  Used when the launch still fills the chip that way.
template <int G>
__global__ void __launch_bounds__(1024) k_sppf_pool3g(const __half *in, int ldi, __half *o1, __half *o2, __half *o3, int ldo,
                                                      int H, int W, int C)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int MAXIT = 4;             // items per thread: HW * G <= 4096
    const int HW = H * W, n = HW * G, cgb = C / (8 * G);
    h8 *x = (h8 *)smem;                  // [HW][G]; holds the 13-wide row maxima after the row pass
    h8 *r5 = x + n, *r9 = r5 + n;
    const int b = blockIdx.x / cgb, gb = blockIdx.x - b * cgb;
    const size_t base = (size_t)b * HW;
    const int c0 = gb * 8 * G;
    for (int q = threadIdx.x; q < n; q += 1024) x[q] = *reinterpret_cast<const h8 *>(in + (base + q / G) * ldi + c0 + (q % G) * 8);
    __syncthreads();
    h8 m13[MAXIT];
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
        const int q = threadIdx.x + it * 1024;
        if (q < n) {
            const int p = q / G, xx = p % W;
            h8 m = x[q];
#pragma unroll
            for (int d = 1; d <= 6; ++d) {
                if (xx - d >= 0) m = __builtin_elementwise_max(m, x[q - d * G]);
                if (xx + d < W) m = __builtin_elementwise_max(m, x[q + d * G]);
                if (d == 2) r5[q] = m;
                if (d == 4) r9[q] = m;
            }
            m13[it] = m;
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
        const int q = threadIdx.x + it * 1024;
        if (q < n) x[q] = m13[it];
    }
    __syncthreads();
    const int WG = W * G;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
        const int q = threadIdx.x + it * 1024;
        if (q < n) {
            const int p = q / G, y = p / W;
            h8 m5 = r5[q], m9 = r9[q], m = x[q];
#pragma unroll
            for (int d = 1; d <= 6; ++d) {
                if (y - d >= 0) {
                    if (d <= 2) m5 = __builtin_elementwise_max(m5, r5[q - d * WG]);
                    if (d <= 4) m9 = __builtin_elementwise_max(m9, r9[q - d * WG]);
                    m = __builtin_elementwise_max(m, x[q - d * WG]);
                }
                if (y + d < H) {
                    if (d <= 2) m5 = __builtin_elementwise_max(m5, r5[q + d * WG]);
                    if (d <= 4) m9 = __builtin_elementwise_max(m9, r9[q + d * WG]);
                    m = __builtin_elementwise_max(m, x[q + d * WG]);
                }
            }
            const size_t o = (base + p) * ldo + c0 + (q % G) * 8;
            *reinterpret_cast<h8 *>(o1 + o) = m5;
            *reinterpret_cast<h8 *>(o2 + o) = m9;
            *reinterpret_cast<h8 *>(o3 + o) = m;
        }
    }
}

}  // namespace

extern "C" int rva_sppf_pool3_nhwc_f16(rva_ctx *ctx, const void *in, int ldi, void *out1, void *out2, void *out3, int ldo, int batch,
                                       int H, int W, int C, rva_stream_t stream_)
{
    if (!ctx || !in || !out1 || !out2 || !out3 || C % 8 || ldi % 8 || ldo % 8 || batch <= 0 || H <= 0 || W <= 0)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_sppf_pool3_nhwc_f16: bad argument");
    const size_t smem = (size_t)H * W * 16 * 4;
    if (smem > 150 * 1024) return rva_fail(ctx, RVA_ERR_ARG, "rva_sppf_pool3_nhwc_f16: H*W too large for one LDS tile (use rva_maxpool5_nhwc_f16 x3)");
    // whole 64-byte runs per wave where that still fills the chip (32 frames of YOLOv8s: 256 blocks of 1024 threads)
    if (C % 32 == 0 && (long)batch * (C / 32) >= 192 && (size_t)H * W * 4 <= 4096 && (size_t)H * W * 4 * 16 * 3 <= 150 * 1024 && !getenv("RVA_SPPF_G1")) {
        RVA_HIP(ctx, rva_func_smem((const void *)k_sppf_pool3g<4>, 150 * 1024));
        k_sppf_pool3g<4><<<batch * (C / 32), 1024, (size_t)H * W * 4 * 16 * 3, (hipStream_t)stream_>>>((const __half *)in, ldi, (__half *)out1,
                                                                                              (__half *)out2, (__half *)out3, ldo, H, W, C);
        RVA_HIP(ctx, hipGetLastError());
        return RVA_OK;
    }
    RVA_HIP(ctx, rva_func_smem((const void *)k_sppf_pool3, 150 * 1024));
    k_sppf_pool3<<<batch * (C / 8), 256, smem, (hipStream_t)stream_>>>((const __half *)in, ldi, (__half *)out1, (__half *)out2,
                                                                       (__half *)out3, ldo, H, W, C);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------------
// Detect head: box logits [B, hw, 4*16] + class logits [B, hw, nc] of one level ->
// out[B, 4+nc, A] at anchor offset a0 (xywh * stride, sigmoid scores).  Thread = anchor.
struct HeadArgs {
    const __half *box; int ldb; const __half *cls; int ldc; __half *out;
    int B, h, w, nc, A, a0; float stride;
};

struct Head3Args { HeadArgs lv[3]; int blocks[3]; };     // blocks[l] = 256-anchor blocks of level l

template <bool BOX32 = false>
__device__ __forceinline__ void head_anchor(const HeadArgs &a, int i, int b, float *box32 = nullptr);

__global__ void __launch_bounds__(256) k_head(HeadArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.h * a.w) head_anchor(a, i, blockIdx.y);
}

// the three pyramid levels in one launch: the two small levels no longer run as separate, under-filled kernels
__global__ void __launch_bounds__(256) k_head3(Head3Args a)
{
    int blk = blockIdx.x, l = 0;
    if (blk >= a.blocks[0]) { blk -= a.blocks[0]; l = 1; if (blk >= a.blocks[1]) { blk -= a.blocks[1]; l = 2; } }
    const HeadArgs &h = a.lv[l];
    const int i = blk * 256 + threadIdx.x;
    if (i < h.h * h.w) head_anchor(h, i, blockIdx.y);
}

// the same launches with the fp32 side tensor box32[B, 4, A] of the box rows (rva_yolo_head_box32_f16 / rva_yolo_head3_box32_f16)
__global__ void __launch_bounds__(256) k_head_box32(HeadArgs a, float *box32)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.h * a.w) head_anchor<true>(a, i, blockIdx.y, box32);
}

__global__ void __launch_bounds__(256) k_head3_box32(Head3Args a, float *box32)
{
    int blk = blockIdx.x, l = 0;
    if (blk >= a.blocks[0]) { blk -= a.blocks[0]; l = 1; if (blk >= a.blocks[1]) { blk -= a.blocks[1]; l = 2; } }
    const HeadArgs &h = a.lv[l];
    const int i = blk * 256 + threadIdx.x;
    if (i < h.h * h.w) head_anchor<true>(h, i, blockIdx.y, box32);
}

template <bool BOX32>
__device__ __forceinline__ void head_anchor(const HeadArgs &a, int i, int b, float *box32)
{
    const int hw = a.h * a.w;
    const size_t pix = (size_t)b * hw + i;
    const __half *bp = a.box + pix * a.ldb;
    float d[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float v[16], mx = -1e30f;
        const uint4 q0 = *reinterpret_cast<const uint4 *>(bp + s * 16), q1 = *reinterpret_cast<const uint4 *>(bp + s * 16 + 8);
        const __half2 *h0 = reinterpret_cast<const __half2 *>(&q0), *h1 = reinterpret_cast<const __half2 *>(&q1);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float2 f = __half22float2(h0[t]); v[2 * t] = f.x; v[2 * t + 1] = f.y;
            f = __half22float2(h1[t]); v[8 + 2 * t] = f.x; v[9 + 2 * t] = f.y;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) mx = fmaxf(mx, v[t]);
        float se = 0.f, sw = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) { const float e = __expf(v[t] - mx); se += e; sw += e * (float)t; }
        d[s] = sw / se;                                  // DFL expectation
    }
    const float ax = (float)(i % a.w) + 0.5f, ay = (float)(i / a.w) + 0.5f;
    const float x1 = ax - d[0], y1 = ay - d[1], x2 = ax + d[2], y2 = ay + d[3];
    __half *o = a.out + (size_t)b * (4 + a.nc) * a.A + a.a0 + i;
    o[0] = __float2half_rn((x1 + x2) * 0.5f * a.stride);
    o[(size_t)a.A] = __float2half_rn((y1 + y2) * 0.5f * a.stride);
    o[(size_t)2 * a.A] = __float2half_rn((x2 - x1) * a.stride);
    o[(size_t)3 * a.A] = __float2half_rn((y2 - y1) * a.stride);
    if constexpr (BOX32) {    // the four values the roundings above took (the same fp32 operations: one value each), anchor axis
        float *o32 = box32 + (size_t)b * 4 * a.A + a.a0 + i;      // contiguous like the fp16 rows
        o32[0] = (x1 + x2) * 0.5f * a.stride;
        o32[(size_t)a.A] = (y1 + y2) * 0.5f * a.stride;
        o32[(size_t)2 * a.A] = (x2 - x1) * a.stride;
        o32[(size_t)3 * a.A] = (y2 - y1) * a.stride;
    }
    // class logits eight at a time from a row of ldc >= roundup(nc, 8) halves; only the class rows < nc exist in `out` (a ragged
    // nc: the row's pad columns are loaded and dropped, whatever they hold)
    const __half *cp = a.cls + pix * a.ldc;
    for (int c = 0; c < a.nc; c += 8) {                  // (uniform branch: whole groups of eight take the unguarded stores)
        const uint4 q = *reinterpret_cast<const uint4 *>(cp + c);
        if (c + 8 <= a.nc) store_scores8<false>(o + (size_t)(4 + c) * a.A, (size_t)a.A, q, 8);
        else store_scores8<true>(o + (size_t)(4 + c) * a.A, (size_t)a.A, q, a.nc - c);
    }
}

}  // namespace

static int yolo_head3(rva_ctx *ctx, const void *const *box_logits, const int32_t *ldb, const void *const *cls_logits,
                      const int32_t *ldc, void *out, float *boxes32, int batch, const int32_t *h, const int32_t *w, int nc, int anchors_total,
                      const float *strides, rva_stream_t stream_, bool any_nc = false)
{
    if (!ctx || !box_logits || !cls_logits || !ldb || !ldc || !h || !w || !strides || !out ||
        (any_nc ? nc < 1 || nc > 1024 || batch <= 0 : nc % 8 != 0))
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head3_f16: bad argument");
    Head3Args a{};
    int a0 = 0, total = 0;
    for (int l = 0; l < 3; ++l) {
        if (!box_logits[l] || !cls_logits[l] || ldb[l] % 8 || ldc[l] % 8 || h[l] <= 0 || w[l] <= 0 || (any_nc && ldc[l] < (nc + 7) / 8 * 8))
            return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head3_f16: bad level %d", l);
        a.lv[l] = HeadArgs{(const __half *)box_logits[l], ldb[l], (const __half *)cls_logits[l], ldc[l], (__half *)out, batch,
                           h[l], w[l], nc, anchors_total, a0, strides[l]};
        a.blocks[l] = rva_ceil_div(h[l] * w[l], 256);
        total += a.blocks[l];
        a0 += h[l] * w[l];
    }
    if (a0 != anchors_total) return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head3_f16: anchors_total != sum of h*w");
    if (boxes32) k_head3_box32<<<dim3(total, batch), 256, 0, (hipStream_t)stream_>>>(a, boxes32);
    else k_head3<<<dim3(total, batch), 256, 0, (hipStream_t)stream_>>>(a);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

// one level, the arguments checked by the caller; boxes32 != NULL: with the fp32 side tensor of the box rows
static int yolo_head1(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc, void *out, float *boxes32, int batch,
                      int h, int w, int nc, int anchors_total, int anchor_offset, float stride, rva_stream_t stream_)
{
    HeadArgs a{(const __half *)box_logits, ldb, (const __half *)cls_logits, ldc, (__half *)out, batch, h, w, nc,
               anchors_total, anchor_offset, stride};
    dim3 g(rva_ceil_div(h * w, 256), batch);
    if (boxes32) k_head_box32<<<g, 256, 0, (hipStream_t)stream_>>>(a, boxes32);
    else k_head<<<g, 256, 0, (hipStream_t)stream_>>>(a);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

extern "C" {

int rva_yolo_head3_f16(rva_ctx *ctx, const void *const *box_logits, const int32_t *ldb, const void *const *cls_logits,
                       const int32_t *ldc, void *out, int batch, const int32_t *h, const int32_t *w, int nc, int anchors_total,
                       const float *strides, rva_stream_t stream_)
{
    return yolo_head3(ctx, box_logits, ldb, cls_logits, ldc, out, nullptr, batch, h, w, nc, anchors_total, strides, stream_);
}

int rva_yolo_head3_box32_f16(rva_ctx *ctx, const void *const *box_logits, const int32_t *ldb, const void *const *cls_logits,
                             const int32_t *ldc, void *out, float *boxes32, int batch, const int32_t *h, const int32_t *w, int nc,
                             int anchors_total, const float *strides, rva_stream_t stream_)
{
    if (!ctx) return RVA_ERR_ARG;
    if (!boxes32 || (uintptr_t)boxes32 % 4) return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head3_box32_f16: boxes32 must be a float tensor [batch, 4, anchors_total]");
    return yolo_head3(ctx, box_logits, ldb, cls_logits, ldc, out, boxes32, batch, h, w, nc, anchors_total, strides, stream_);
}

int rva_yolo_head3_nc_f16(rva_ctx *ctx, const void *const *box_logits, const int32_t *ldb, const void *const *cls_logits,
                          const int32_t *ldc, void *out, float *boxes32, int batch, const int32_t *h, const int32_t *w, int nc,
                          int anchors_total, const float *strides, rva_stream_t stream_)
{
    if (!ctx) return RVA_ERR_ARG;
    if ((uintptr_t)boxes32 % 4) return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head3_nc_f16: boxes32 must be NULL or a float tensor [batch, 4, anchors_total]");
    return yolo_head3(ctx, box_logits, ldb, cls_logits, ldc, out, boxes32, batch, h, w, nc, anchors_total, strides, stream_, true);
}

int rva_yolo_head_nc_f16(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc, void *out, float *boxes32,
                         int batch, int h, int w, int nc, int anchors_total, int anchor_offset, float stride, rva_stream_t stream_)
{
    if (!ctx) return RVA_ERR_ARG;
    if (!box_logits || !cls_logits || !out || (uintptr_t)boxes32 % 4 || nc < 1 || nc > 1024 || ldb % 8 || ldc % 8 || ldc < (nc + 7) / 8 * 8 ||
        batch <= 0 || h <= 0 || w <= 0 || anchor_offset < 0 || anchor_offset + h * w > anchors_total)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head_nc_f16: bad argument (1 <= nc <= 1024; ldb, ldc %% 8; ldc >= roundup(nc, 8); the level inside "
                        "the anchor range)");
    return yolo_head1(ctx, box_logits, ldb, cls_logits, ldc, out, boxes32, batch, h, w, nc, anchors_total, anchor_offset, stride, stream_);
}

int rva_yolo_head_f16(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc, void *out, int batch,
                      int h, int w, int nc, int anchors_total, int anchor_offset, float stride, rva_stream_t stream_)
{
    if (!ctx) return RVA_ERR_ARG;
    if (!box_logits || !cls_logits || !out || nc % 8 || ldb % 8 || ldc % 8 || batch <= 0 || h <= 0 || w <= 0 || anchor_offset < 0 ||
        anchor_offset + h * w > anchors_total)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head_f16: bad argument (nc, ldb, ldc %% 8; the level inside the anchor range)");
    return yolo_head1(ctx, box_logits, ldb, cls_logits, ldc, out, nullptr, batch, h, w, nc, anchors_total, anchor_offset, stride, stream_);
}

int rva_yolo_head_box32_f16(rva_ctx *ctx, const void *box_logits, int ldb, const void *cls_logits, int ldc, void *out, float *boxes32,
                            int batch, int h, int w, int nc, int anchors_total, int anchor_offset, float stride, rva_stream_t stream_)
{
    if (!ctx) return RVA_ERR_ARG;
    if (!box_logits || !cls_logits || !out || !boxes32 || (uintptr_t)boxes32 % 4 || nc % 8 || ldb % 8 || ldc % 8 || batch <= 0 || h <= 0 || w <= 0 ||
        anchor_offset < 0 || anchor_offset + h * w > anchors_total)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo_head_box32_f16: bad argument (boxes32 [batch, 4, anchors_total] float, the level inside the anchor range)");
    return yolo_head1(ctx, box_logits, ldb, cls_logits, ldc, out, boxes32, batch, h, w, nc, anchors_total, anchor_offset, stride, stream_);
}

}  // extern "C"
