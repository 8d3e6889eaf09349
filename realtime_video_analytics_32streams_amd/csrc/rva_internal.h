// Internal definitions shared by the librva translation units (not part of the C ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "rva.h"

struct rva_resize_table {  // device copy of the per-axis resize taps for one geometry
    int32_t *ofs = nullptr;   // [n]   first source index
    int16_t *w0 = nullptr;    // [n]   11-bit fixed-point weight of tap 0
    int16_t *w1 = nullptr;    // [n]   ... of tap 1
    int n = 0;
};

struct rva_geom_cache {
    rva_resize_table x, y;
};

struct rva_jpeg_state;           // scratch of the device JPEG encoder (rva_jpeg.hip)

struct rva_ctx {
    int device = 0;
    rva_jpeg_state *jpeg = nullptr;
    std::string err;
    // post-process scratch, sized by rva_reserve / grown on demand
    int cap_batch = 0, cap_anchors = 0;
    float *sp_box = nullptr;      // [B][A][4] xyxy of thresholded anchors (sparse, anchor-indexed)
    float *sp_score = nullptr;    // [B][A]
    int32_t *sp_cls = nullptr;    // [B][A]
    uint32_t *cand_bits = nullptr;// [B][ceil(A/32)] pass bitmap in anchor order
    int32_t *post_flags = nullptr;// [2 + RVA_MAX_BATCH]: overflow flags, K2's improper-box flag per image of the launch, images NMS'd with the centre-bin filter
    // resize tap tables keyed by (src, dst) per axis
    std::map<uint64_t, rva_resize_table> taps_x, taps_y;
    // one-shot profiling events for the next K1 (integer-ratio) launch: rva_profile_next_preprocess
    hipEvent_t k1_start = nullptr, k1_stop = nullptr;
    int k1_px = -1;               // RVA_K1_PX tuning switch, read once per context
    int k1_nt = -1;               // RVA_K1_NT experiment switch (non-temporal loads / stores in the steady-state K1), read once per context
    int num_cus = 0;              // multiProcessorCount of ctx->device (persistent-grid sizing)
};

inline int rva_fail(rva_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define RVA_HIP(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return rva_fail((ctx), RVA_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                                    \
    } while (0)

// Host restatement of the OpenCV resize tap computation; fills a device table (cached in ctx).
int rva_get_taps(rva_ctx *ctx, int src, int dst, bool is_x, rva_resize_table *out);

static inline int rva_ceil_div(int a, int b) { return (a + b - 1) / b; }

// The output row window [y0, y1) of entry point `who` (a *_rows function) in an image of Ho output rows: y1 < 0 = the last row.
inline int rva_row_window(rva_ctx *ctx, const char *who, int y0, int &y1, int Ho)
{
    if (y1 < 0) y1 = Ho;
    if (y0 < 0 || y0 >= y1 || y1 > Ho) return rva_fail(ctx, RVA_ERR_ARG, "%s: rows [%d, %d) are not a window of %d output rows", who, y0, y1, Ho);
    return RVA_OK;
}

// Raise a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) to at least `bytes` on the CURRENT
// device.  The attribute belongs to the (device, function) pair, so the bookkeeping is keyed by both: a second context
// on another device of the same process gets its own call (a process-global `static bool` would skip it).  Must not be
// reached for the first time inside a stream capture: callers run one eager launch of every kernel before capturing.
hipError_t rva_func_smem(const void *fn, size_t bytes);

// multiProcessorCount of ctx->device, read once into ctx->num_cus (256 if the query fails)
int rva_num_cus(rva_ctx *ctx);

// true for the variants of rva_conv2d_nhwc_f16_v that the fused 1x1 forms (rva_conv1x1_upcat_f16, rva_conv1x1_head_*) also take
bool rva_conv_variant_is_gather64(int variant);
// fp16 variants whose kernel takes an output row window (rva_conv2d_nhwc_f16_rows); variant 0 by the shape it would pick for
bool rva_conv_variant_rows(int variant, int Cin, int ksize, int stride);

// rva_conv2d_nhwc_f16_rows on the `batch` leading images of buffers that hold sel_batch (>= batch): variant 0 chooses its kernel
// from sel_batch, so that the kernel -- and with it every bit of an image -- does not depend on how many images a call runs
int rva_conv2d_nhwc_f16_sel(rva_ctx *ctx, const void *in, int ldi, const void *weights, const float *bias, void *out, int ldo,
                            const void *residual, int ldr, int batch, int sel_batch, int H, int W, int Cin, int Cout, int ksize, int stride,
                            int act, int variant, int y0, int y1, rva_stream_t stream);

// frees ctx->jpeg (rva_jpeg.hip); called by rva_destroy
void rva_jpeg_free(rva_ctx *ctx);

// ---------------------------------------------------------------------------------------------------
// The host scaffold of the clip and classifier plans (rva_clip.hip, rva_clip_f16.hip, rva_clip3d.hip, rva_resnet*.hip).  The fp32
// and the fp16 form of a plan share everything here; a plan file keeps only what differs by precision: element types, rounding,
// kernels, launches.  The networks' own shapes (ResNet topology, 3D-CNN geometry, CNN-LSTM maps and stages) are in rva_plan_topo.h;
// the CNN-LSTM's host plan over both precisions is rva_clip_host.h, the bodies of its K_xproj / K_lstm rva_lstm_dev.h.

// Device memory of a plan: every buffer is an array of `n` elements of T owned until release().
struct rva_dev_arena {
    std::vector<void *> allocs;

    template <typename T>
    int alloc(rva_ctx *ctx, T **dst, size_t n)
    {
        void *m = nullptr;
        RVA_HIP(ctx, hipMalloc(&m, std::max<size_t>(n, 1) * sizeof(T)));
        allocs.push_back(m);
        *dst = (T *)m;
        return RVA_OK;
    }

    template <typename T>
    int upload(rva_ctx *ctx, T **dst, const T *src, size_t n)
    {
        const int rc = alloc(ctx, dst, n);
        if (rc != RVA_OK) return rc;
        RVA_HIP(ctx, hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
        return RVA_OK;
    }

    void release()
    {
        for (void *m : allocs) (void)hipFree(m);
        allocs.clear();
    }
};

// What a plan's create refuses before it allocates anything: RVA_ERR_CAPACITY if `need` bytes exceed the free device memory (or
// it cannot be read).  `shape` is the formatted phrase that names the capacity ("8 clips of 16 x 112 x 112").  In rva_clip.hip.
int rva_plan_fits(rva_ctx *ctx, const char *who, size_t need, const char *shape);

constexpr int RVA_PLAN_MAX_CLASSES = 16384;                // the top-k kernel keeps a row's logits in LDS

// output length of a stride-2 window (k, pad) over n; the stem's maps: conv 7x7 s2 p3 (Hc x Wc), then max pool 3x3 s2 p1 (Hp x Wp)
inline int rva_half_map(int n, int k, int pad) { return (n + 2 * pad - k) / 2 + 1; }
inline void rva_stem_maps(int H, int W, int *Hc, int *Wc, int *Hp, int *Wp)
{
    *Hc = rva_half_map(H, 7, 3); *Wc = rva_half_map(W, 7, 3);
    *Hp = rva_half_map(*Hc, 3, 1); *Wp = rva_half_map(*Wc, 3, 1);
}

// a 3x3 convolution's weights [co][ci][ky][kx] -> [co][tap][ci], what the MFMA tap loops read
template <typename T>
std::vector<T> rva_pack_taps_major(const T *w, int cout, int cin)
{
    std::vector<T> out((size_t)cout * 9 * cin);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t) out[((size_t)co * 9 + t) * cin + ci] = w[((size_t)co * cin + ci) * 9 + t];
    return out;
}

// The stem (Conv 7x7 s2 p3 + bias + ReLU + MaxPool 3x3 s2 p1 from planar fp32 frames read through a frame-index table, NHWC
// out: `pooled` = [n_frames][Hp][Wp][64]), mean (tile partials in tile order / n; `rows` blocks of `channels` threads), head
// (Linear: one thread per class, k in order) and top-k (rank counting, the first k ranks, 1 <= k <= classes) kernels of the clip
// plans, defined in rva_clip.hip and shared by rva_clip3d.hip and rva_resnet.hip.  *_prepare raises the kernel's dynamic-LDS limit
// (at plan creation, never inside a capture); *_launch only launches on `st`.  `who` names the ABI entry in the argument error
// of the top-k launch.
int rva_clip_stem_prepare(rva_ctx *ctx);
int rva_clip_stem_launch(rva_ctx *ctx, const float *frames, const int32_t *frame_index, const float *w1, const float *b1, float *pooled,
                         int H, int W, int n_frames, hipStream_t st);
int rva_clip_mean_launch(rva_ctx *ctx, const float *partial, int tiles, float n, float *feat, int rows, int channels, hipStream_t st);
int rva_clip_head_prepare(rva_ctx *ctx, int hidden);
int rva_clip_head_launch(rva_ctx *ctx, const float *x, const float *wh, const float *bh, float *logits, int hidden, int classes,
                         int n_clips, hipStream_t st);
int rva_clip_post_prepare(rva_ctx *ctx, int classes);
int rva_clip_post_launch(rva_ctx *ctx, const char *who, const float *logits, int classes, int k, const int32_t *rows, int n_rows,
                         int max_det, float *scores, int32_t *cls, float *boxes, int32_t *counts, hipStream_t st);

// The fp16 stem of rva_clip_f16.hip (K_stem: the same network stage on v_mfma_f32_32x32x16_f16 from planar fp16 frames, `pooled`
// fp16 NHWC with one rounding), shared with rva_resnet_f16.hip.  rva_round_f16 (every fp16 plan's weight rounding): `n` fp32
// values rounded once to fp16 (to nearest even), false if one does not stay finite.  rva_clip16_stem_pack: the rounded conv1 weights [64][3][7][7] in the kernel's layout
// (what `w1` of the launch points to, on the device).
bool rva_round_f16(const float *src, size_t n, std::vector<_Float16> &dst);
std::vector<_Float16> rva_clip16_stem_pack(const std::vector<_Float16> &c1);
int rva_clip16_stem_prepare(rva_ctx *ctx);
int rva_clip16_stem_launch(rva_ctx *ctx, const _Float16 *frames, const int32_t *frame_index, const _Float16 *w1, const float *b1,
                           _Float16 *pooled, int H, int W, int n_frames, hipStream_t st);

// K_mean of the ResNet plans (rva_resnet.hip): feat[img][c] = (the image's P pixels of x [n][P][C] in raster order, from zero) / P;
// C a multiple of 256
int rva_res_mean_launch(rva_ctx *ctx, const float *x, int P, int C, float *feat, int n, hipStream_t st);

// The tail of every *_plan_stage tap: reports `count` through n_elems, and if dst is given checks its size and copies `count`
// elements of `esize` bytes device to device on `st` -- as `rows` rows of row_elems out of a pitch of pitch_elems if rows > 0,
// else flat.  `unit` ("floats" / "elements") and `items` ("clips" / "frames") are the words of the ABI entry's size error.
int rva_clip_stage_copy(rva_ctx *ctx, const char *who, int stage, int n, const char *items, const void *src, size_t esize,
                        const char *unit, int64_t count, int64_t rows, int64_t row_elems, int64_t pitch_elems, void *dst,
                        int64_t dst_elems, int64_t *n_elems, hipStream_t st);
