// fp32 ResNet-18 classifier (classify.ResNet18: the reference's ResNet head, detector.py:870-1001) as one plan object:
//
//   per frame [3,H,W]: Conv 7x7 s2 p3 + BN + ReLU -> MaxPool 3x3 s2 p1 -> 8 BasicBlocks (64, 64, 128, 128, 256, 256, 512, 512; the
//                      first block of the 128 / 256 / 512 stages has stride 2 and a 1x1 stride-2 shortcut convolution)
//                      -> mean over H,W -> Linear(512 -> classes) -> top-k
//
// Everything is fp32 (BatchNorm is folded by the caller in float64 and rounded once); activations are NHWC.  The contracts are
// those of rva_clip.hip: every sum runs in ONE fixed order that depends neither on the number of frames, nor on a frame's position
// in the batch, nor on the tile shape, nor on the launch mode -- no split-K and no float atomics -- so logits are bit-identical
// across batch sizes, batch rows, an index-table permutation of the frames, eager launches and hipGraph replay.  The launches of
// one pass (rva_resnet_plan_run), all on the caller's stream:
//
//   K_stem   k_clip_stem of rva_clip.hip through rva_clip_stem_launch: conv1 + bias + ReLU + max pool from the planar frames
//            (read through the device table of frame indices), NHWC out.
//   K_conv   x 19: k_res_conv, the NHWC implicit GEMM of a block convolution on the exact fp32-input MFMA core of
//            rva_mfma_f32.h (which defines the reduction order: what rva_conv2d_nhwc_f32_v runs on the same input).  Rows = output
//            pixels of the whole batch, columns = output channels.  Per block: mid = ReLU(conv1(x) + b), [down = conv_d(x) + b],
//            out = ReLU((conv2(mid) + b) + (down or x)).
//   K_mean   k_res_mean through rva_res_mean_launch (shared with rva_resnet_f16.hip): per image and channel the pixels in raster
//            order from zero, then one division by h*w.
//   K_head   Linear: the head kernel of rva_clip.hip (one thread per class, k in order), hidden = 512.
//   K_post   (rva_resnet_plan_run_post) the top-k kernel of rva_clip.hip with the descriptor's k.
//
// Every stage keeps its own workspace buffer (rva_resnet_plan_stage reads them).  The launches come from the one ResNet topology
// of rva_plan_topo.h with the ResNet-18 descriptor (rva_res18_desc); the tap translates its stage code (rva_res18_stage).
#include "rva_mfma_f32.h"
#include "rva_plan_topo.h"

namespace {

struct ResConvArgs {
    const float *in;                 // [n][H][W][Cin]
    const float *w;                  // [Cout][KS*KS][Cin]
    const float *bias;               // [Cout]
    const float *res;                // [n][Ho][Wo][Cout] (EPI_RES_RELU)
    float *out;                      // [n][Ho][Wo][Cout]
    int H, W, Ho, Wo, Cin, Cout, stride, epi;
    long M;                          // n * Ho * Wo
};

// ---------------------------------------------------------------------------------------------------
// K_conv.  MT x NT tiles of 32 x 32 per wave, WM x WN waves per block: block = 32 MT WM pixels x 32 NT WN channels (Cout is a
// multiple of it: no column tail).  KS = 3 (pad 1) or 1 (pad 0).  Row p of the GEMM = pixel (p / (Ho Wo), (p / Wo) % Ho, p % Wo) of
// the batch, so a tile may span two images; rows >= M read nothing and write nothing.  Reduction: taps in order, channels in
// chunks of 32, f32_chunk's step order, from zero.  Epilogues: max(acc + bias, 0) | acc + bias | max((acc + bias) + res, 0).
template <int MT, int NT, int WM, int WN, int KS>
__global__ void __launch_bounds__(64 * WM * WN) k_res_conv(ResConvArgs a)
{
    constexpr int CK = 32, PAD = KS / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int r = lane & 31, h = lane >> 5;
    const long m0 = ((long)blockIdx.x * WM + wm) * (32 * MT);
    const int n0 = (blockIdx.y * WN + wn) * (32 * NT);

    int pn[MT], py[MT], px[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        long p = m0 + mt * 32 + r;
        pv[mt] = p < a.M;
        if (!pv[mt]) p = 0;
        px[mt] = (int)(p % a.Wo);
        py[mt] = (int)((p / a.Wo) % a.Ho);
        pn[mt] = (int)(p / ((long)a.Wo * a.Ho));
    }
    const float *wrow[NT];
    bool wv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        wv[nt] = true;
        wrow[nt] = a.w + (size_t)(n0 + nt * 32 + r) * (KS * KS) * a.Cin + (CK / 2) * h;
    }
    f32x16 acc[MT][NT] = {};
    for (int tap = 0; tap < KS * KS; ++tap) {
        const int ky = tap / KS, kx = tap - ky * KS;
        const float *arow[MT];
        bool av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int iy = py[mt] * a.stride + ky - PAD, ix = px[mt] * a.stride + kx - PAD;
            av[mt] = pv[mt] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            arow[mt] = a.in + ((size_t)((long)pn[mt] * a.H + (av[mt] ? iy : 0)) * a.W + (av[mt] ? ix : 0)) * a.Cin + (CK / 2) * h;
        }
        const size_t wtap = (size_t)tap * a.Cin;
        for (int c = 0; c < a.Cin; c += CK) f32_chunk<MT, NT, CK>(acc, arow, av, c, wrow, wv, wtap + c);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + nt * 32 + r;
        const float bias = a.bias[co];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long p = m0 + mt * 32 + f32_cd_row(i, h);
                if (p >= a.M) continue;
                const size_t o = (size_t)p * a.Cout + co;
                float v = acc[mt][nt][i] + bias;
                if (a.epi == EPI_RES_RELU) v = v + a.res[o];
                if (a.epi != EPI_BIAS) v = fmaxf(v, 0.f);
                a.out[o] = v;
            }
        }
    }
}

// The tile table: (MT, NT, WM, WN) -> block of (32 MT WM) pixels x (32 NT WN) channels, largest first.  The wide layers (many
// rows) take the 2 x 2 tiles per wave (four accumulators, a quarter of the operand traffic per MFMA); the deep layers (few rows,
// long K) take one tile per wave in small blocks so the grid still covers the device.
struct ResTile { int mt, nt, wm, wn; };
constexpr ResTile kResTiles[] = {
    {2, 2, 4, 1},    // 0: 256 x 64
    {1, 2, 4, 1},    // 1: 128 x 64
    {1, 1, 2, 2},    // 2: 64 x 64
    {1, 1, 1, 2},    // 3: 32 x 64
};
constexpr int kNumResTiles = (int)(sizeof kResTiles / sizeof kResTiles[0]);

dim3 res_grid(int v, long M, int Cout)
{
    const ResTile &t = kResTiles[v];
    return dim3((unsigned)((M + 32L * t.mt * t.wm - 1) / (32L * t.mt * t.wm)), (unsigned)(Cout / (32 * t.nt * t.wn)));
}

// the largest tile that still gives every CU a block, else the smallest
int res_tile_for(long M, int Cout, int num_cus)
{
    const long want = num_cus > 0 ? num_cus : 256;
    for (int v = 0; v < kNumResTiles; ++v) {
        const dim3 g = res_grid(v, M, Cout);
        if ((long)g.x * g.y >= want) return v;
    }
    return kNumResTiles - 1;
}

template <int KS>
void launch_res_conv(int v, dim3 g, hipStream_t st, const ResConvArgs &a)
{
    switch (v) {
    case 0: k_res_conv<2, 2, 4, 1, KS><<<g, 256, 0, st>>>(a); break;
    case 1: k_res_conv<1, 2, 4, 1, KS><<<g, 256, 0, st>>>(a); break;
    case 2: k_res_conv<1, 1, 2, 2, KS><<<g, 256, 0, st>>>(a); break;
    default: k_res_conv<1, 1, 1, 2, KS><<<g, 128, 0, st>>>(a); break;
    }
}

// ---------------------------------------------------------------------------------------------------
// K_mean for any channel count that is a multiple of 256.  Block = (image, 256 channels), thread = channel:
// feat[img][c] = (sum of the image's P pixels in raster order, from zero) / P.
__global__ void __launch_bounds__(256) k_res_mean(const float *x, int P, int C, float *feat)
{
    const int img = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    const float *xp = x + (size_t)img * P * C + c;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s = s + xp[(size_t)p * C];
    feat[(size_t)img * C + c] = s / (float)P;
}

}  // namespace

int rva_res_mean_launch(rva_ctx *ctx, const float *x, int P, int C, float *feat, int n, hipStream_t st)
{
    k_res_mean<<<dim3(n, C / 256), 256, 0, st>>>(x, P, C, feat);
    RVA_HIP(ctx, hipGetLastError());
    return RVA_OK;
}

struct rva_resnet_plan {
    rva_ctx *ctx = nullptr;
    rva_resnet_desc d{};
    int k = 0;                                             // min(top_k, classes)
    rva_res_topo t;                                        // of rva_res18_desc(d)
    float *ws = nullptr, *bs = nullptr, *wh = nullptr, *bh = nullptr;
    float *w[RES_CONVS] = {}, *b[RES_CONVS] = {};          // of rva_resnet_weights::conv[i]
    std::vector<float *> stage;                            // every stage keeps its own buffer, indexed by the topology's stage code
    size_t workspace_bytes = 0;
    rva_dev_arena mem;
};

extern "C" {

int rva_resnet_plan_create(rva_ctx *ctx, const rva_resnet_desc *desc, const rva_resnet_weights *wt, rva_resnet_plan **out)
{
    int rc = rva_res_check_args(ctx, "rva_resnet_plan_create", desc, wt, (void **)out);
    if (rc != RVA_OK) return rc;
    const rva_resnet_desc d = *desc;
    const rva_res_topo t = rva_res_topology(rva_res18_desc(d));
    const size_t mf = (size_t)d.max_frames;
    // sizes first: the workspace must fit before anything is allocated
    size_t n_act = 0, n_w = (size_t)RES_C_STEM * 147 + RES_C_STEM + (size_t)d.classes * (RES_C_FEAT + 1);
    for (int64_t e : t.elems) n_act += mf * e;
    for (int i = 0; i < RES_CONVS; ++i) n_w += t.conv_weights[i] + t.conv_cout[i];
    char shape[64];
    snprintf(shape, sizeof shape, "%d frames of %d x %d", d.max_frames, d.height, d.width);
    rc = rva_plan_fits(ctx, "rva_resnet_plan_create", (n_act + n_w) * sizeof(float), shape);
    if (rc != RVA_OK) return rc;
    auto *p = new rva_resnet_plan();
    p->ctx = ctx;
    p->d = d;
    p->k = std::min(d.top_k, d.classes);
    p->t = t;
    p->workspace_bytes = n_act * sizeof(float);
    p->stage.assign(t.elems.size(), nullptr);
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    step(p->mem.upload(ctx, &p->ws, wt->stem_w, (size_t)RES_C_STEM * 147));
    step(p->mem.upload(ctx, &p->bs, wt->stem_b, RES_C_STEM));
    step(p->mem.upload(ctx, &p->wh, wt->head_w, (size_t)d.classes * RES_C_FEAT));
    step(p->mem.upload(ctx, &p->bh, wt->head_b, d.classes));
    for (size_t s = 0; s < t.elems.size(); ++s)
        if (t.elems[s]) step(p->mem.alloc(ctx, &p->stage[s], mf * t.elems[s]));
    for (int i = 0; i < RES_CONVS; ++i) {
        step(p->mem.upload(ctx, &p->w[i], wt->conv[i].w, t.conv_weights[i]));
        step(p->mem.upload(ctx, &p->b[i], wt->conv[i].b, t.conv_cout[i]));
    }
    if (rc == RVA_OK) rc = rva_clip_stem_prepare(ctx);
    if (rc == RVA_OK) rc = rva_clip_head_prepare(ctx, RES_C_FEAT);
    if (rc == RVA_OK) rc = rva_clip_post_prepare(ctx, d.classes);
    if (rc != RVA_OK) {
        rva_resnet_plan_destroy(p);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

void rva_resnet_plan_destroy(rva_resnet_plan *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

int rva_resnet_plan_info(const rva_resnet_plan *p, int32_t *maps, int64_t *workspace_bytes, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    rva_res_info(p->t, p->workspace_bytes, maps, workspace_bytes, n_launches);
    return RVA_OK;
}

int rva_resnet_plan_run(rva_resnet_plan *p, const void *frames, const int32_t *frame_index, int n, void *logits, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n < 1 || n > p->d.max_frames)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_plan_run: bad argument (n %d, capacity %d)", n, p->d.max_frames);
    const hipStream_t st = (hipStream_t)stream_;
    float *const *buf = p->stage.data();
    int rc = rva_clip_stem_launch(ctx, (const float *)frames, frame_index, p->ws, p->bs, buf[RVA_RESX_POOLED], p->d.height, p->d.width, n, st);
    if (rc != RVA_OK) return rc;
    const int cus = rva_num_cus(ctx);
    for (const rva_res_conv &l : p->t.conv) {
        ResConvArgs a{};
        a.in = buf[l.in]; a.w = p->w[l.wi]; a.bias = p->b[l.wi]; a.res = l.res >= 0 ? buf[l.res] : nullptr; a.out = buf[l.out];
        a.H = l.H; a.W = l.W; a.Ho = l.Ho; a.Wo = l.Wo; a.Cin = l.cin; a.Cout = l.cout; a.stride = l.stride; a.epi = l.epi;
        a.M = (long)n * l.Ho * l.Wo;
        const int v = res_tile_for(a.M, l.cout, cus);
        const dim3 g = res_grid(v, a.M, l.cout);
        if (l.k == 3) launch_res_conv<3>(v, g, st, a);
        else launch_res_conv<1>(v, g, st, a);
        RVA_HIP(ctx, hipGetLastError());
    }
    rc = rva_res_mean_launch(ctx, buf[p->t.last_out], p->t.maps[4][0] * p->t.maps[4][1], RES_C_FEAT, buf[RVA_RESX_FEAT], n, st);
    if (rc != RVA_OK) return rc;
    return rva_clip_head_launch(ctx, buf[RVA_RESX_FEAT], p->wh, p->bh, (float *)logits, RES_C_FEAT, p->d.classes, n, st);
}

int rva_resnet_plan_run_post(rva_resnet_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                             void *cls, void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, "rva_resnet_plan_run_post", (const float *)logits, p->d.classes, p->k, rows, n_rows, max_det,
                                (float *)scores, (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  Every tensor is frame-major NHWC.  (The
// size error counts "clips": this entry's text since it shared the clip plans' tap.)
int rva_resnet_plan_stage(rva_resnet_plan *p, int stage, int n, void *dst, int64_t dst_floats, int64_t *n_floats, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (n < 1 || n > p->d.max_frames)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_plan_stage: bad argument (n %d, capacity %d)", n, p->d.max_frames);
    const int code = rva_res18_stage(stage);
    if (code < 0) return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_plan_stage: unknown stage %d", stage);
    return rva_clip_stage_copy(ctx, "rva_resnet_plan_stage", stage, n, "clips", p->stage[code], sizeof(float), "floats",
                               n * p->t.elems[code], 0, 0, 0, dst, dst_floats, n_floats, (hipStream_t)stream_);
}

}  // extern "C"

