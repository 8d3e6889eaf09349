// The ResNet-18 classifier of rva_resnet.hip for `half: true` (engine "resnet-f16"): the same network, launches and taps, with
// fp16 frames, fp16 convolution weights and fp16 stored activations, and every sum in fp32.  The numeric contract is that of
// clip-f16 / clip3d-f16:
//
//   * input: planar fp16 frames [3][H][W] (what rva_preprocess_frames_* writes for RVA_F16 with RVA_NORM_IMAGENET_F32), read
//     through the device table of frame indices, element by element: nothing is assumed about the alignment of a frame row
//     (odd widths);
//   * weights: every convolution arrives with its BatchNorm folded by the caller in float64; rva_resnet_f16_plan_create rounds
//     stem_w and the 19 conv[i].w once to fp16 (round to nearest even; a value that does not stay finite is refused, naming its
//     array).  All biases, head weight and head bias stay fp32;
//   * stored activations: `pooled`, mid0..7, down2/4/6 and out0..6 are fp16 NHWC with ONE rounding, of the fp32 epilogue value.
//     out7 is fp32 (it feeds only the mean); feat, logits and top-k scores are fp32;
//   * every sum accumulates in fp32 in ONE fixed order, that of rva_mfma_f16.h: taps in order, input channels in chunks of 16, one
//     MFMA per chunk, from zero.  The order depends on nothing but the layer -- not on the number of frames, a frame's row, the
//     tile picked for the launch or the launch mode: no split-K of any kind and no float atomics, so logits are bit-identical
//     across all of those.
//
// The launches of one pass (rva_resnet_f16_plan_run), all on the caller's stream:
//
//   K_stem   k_clip16_stem of rva_clip_f16.hip through rva_clip16_stem_launch: conv1 + bias + ReLU + max pool, fp16 NHWC out.
//   K_conv   x 19: k_res16_conv, the NHWC implicit GEMM of a block convolution on v_mfma_f32_32x32x16_f16.  GEMM rows (the A
//            operand) = output channels, GEMM columns (the B operand) = output pixels of the whole batch, so a tile may span two
//            images; pixels >= M read nothing and write nothing.  KS = 3 (pad 1) or 1 (pad 0), stride 1 or 2.  A lane's
//            activation operand of a chunk is one 16-byte channels-last load (lane half h: channels c + 8h .. c + 8h + 7),
//            fetched one step ahead of its use; the activations do not go through LDS (a pixel's 64 channels of a step are one
//            128-byte line and every wave of a block reads other pixels: there is nothing to share).  The block's weights do: a
//            step is one tap x 64 input channels, its [32 NT][64] weights are fetched into registers during the step before and
//            written to the other of two LDS buffers after that step's MFMAs, with the slot swizzle of f16_conv_taps_wlds (slot q
//            of row `row` at q ^ ((row >> 1) & 7): the 16 rows of a ds_read_b128 lane group fall on 16 different bank positions),
//            one __syncthreads per step.  Every tile but the 2 x 2 one takes steps of 128 channels where Cin allows (rows of 256 bytes,
//            slot q at q ^ (row & 15)): the same chunks in the same order, half the barriers, twice the bytes in flight.  With channels on the accumulator's rows, registers 4j .. 4j+3 of a lane are four
//            consecutive channels of its pixel: the epilogue is one 8-byte fp16 store (16-byte fp32 for out7) per group, and the
//            residual one 8-byte load.  Epilogues, in fp32: max(acc + b, 0) | acc + b | max((acc + b) + res, 0) with res read as
//            fp16 and widened; then one conversion to fp16, or none for out7.
//   K_mean / K_head / K_post: k_res_mean (rva_resnet.hip) and the head and top-k kernels of rva_clip.hip, unchanged.
//
// Every stage keeps its own workspace buffer (rva_resnet_f16_plan_stage reads them).
#include "rva_internal.h"
#include "rva_mfma_f16.h"

#include <cmath>

namespace {

constexpr int C_STEM = 64, C_FEAT = 512, N_BLOCKS = 8, N_CONVS = 19;
constexpr int MAX_CLASSES = 16384;
constexpr int EPI_RELU = 0, EPI_BIAS = 1, EPI_RES_RELU = 2;

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct Res16Args {
    const _Float16 *in;              // [n][H][W][Cin]
    const _Float16 *w;               // [Cout][KS*KS][Cin]
    const float *bias;               // [Cout]
    const _Float16 *res;             // [n][Ho][Wo][Cout] (EPI_RES_RELU)
    void *out;                       // [n][Ho][Wo][Cout], fp16 or (out_f32) fp32
    int H, W, Ho, Wo, Cin, Cout, stride, epi, out_f32;
    long M;                          // n * Ho * Wo
};

// ---------------------------------------------------------------------------------------------------
// K_conv.  A wave owns MT tiles of 32 pixels x NT tiles of 32 channels; the WM waves of a block share the 32 NT channels (their
// weights go through LDS once per block) and take consecutive runs of 32 MT pixels: block = 32 MT WM pixels x 32 NT channels.
// A step is KB = 64 or 128 input channels (four or eight MFMA chunks); Cin is a multiple of KB and Cout of 32 NT: no K tail and no
// channel tail.  The chunks run in the same order for either KB.
template <int MT, int NT, int WM, int KS, int KB>
__global__ void __launch_bounds__(64 * WM) k_res16_conv(Res16Args a)
{
    constexpr int TAPS = KS * KS, PAD = KS / 2, ROWS = 32 * NT, THREADS = 64 * WM;
    constexpr int SW = KB == 64 ? 1 : 0, SM = KB / 8 - 1;     // slot q of row `row` lives at q ^ ((row >> SW) & SM)
    constexpr int PER = ROWS * (KB / 8) / THREADS;           // 16-byte weight slots a thread stages per step
    static_assert(PER * THREADS == ROWS * (KB / 8), "the threads cover a step's weights in whole slots");
    __shared__ __attribute__((aligned(16))) _Float16 wl[2][ROWS * KB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int swz = (r >> SW) & SM;                          // of rows nt * 32 + r, for every nt
    const long m0 = ((long)blockIdx.x * WM + wave) * (32 * MT);
    const int n0 = blockIdx.y * ROWS;
    const int nkb = a.Cin / KB, steps = TAPS * nkb;

    int py[MT], px[MT];
    size_t pimg[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        long p = m0 + mt * 32 + r;
        pv[mt] = p < a.M;
        if (!pv[mt]) p = 0;
        px[mt] = (int)(p % a.Wo) * a.stride - PAD;
        py[mt] = (int)((p / a.Wo) % a.Ho) * a.stride - PAD;
        pimg[mt] = (size_t)(p / ((long)a.Wo * a.Ho)) * a.H * a.W;
    }
    const _Float16 *wblk = a.w + (size_t)n0 * TAPS * a.Cin;

    f16x8 st[PER], fx[KB / 16][MT], fn[KB / 16][MT];
    auto load_w = [&](int tap, int kb) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int s = tid + THREADS * j, row = s / (KB / 8), q = s % (KB / 8);
            st[j] = *reinterpret_cast<const f16x8 *>(wblk + ((size_t)row * TAPS + tap) * a.Cin + kb * KB + q * 8);
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int s = tid + THREADS * j, row = s / (KB / 8), q = s % (KB / 8);
            *reinterpret_cast<f16x8 *>(&wl[buf][row * KB + ((q ^ ((row >> SW) & SM)) << 3)]) = st[j];
        }
    };
    auto load_x = [&](int tap, int kb, f16x8 (&f)[KB / 16][MT]) {
        const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int iy = py[mt] + ky, ix = px[mt] + kx;
            const bool av = pv[mt] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const _Float16 *arow = a.in + (pimg[mt] + (size_t)(av ? iy : 0) * a.W + (av ? ix : 0)) * a.Cin + kb * KB + 8 * h;
#pragma unroll
            for (int c = 0; c < KB / 16; ++c) f[c][mt] = av ? *reinterpret_cast<const f16x8 *>(arow + 16 * c) : f16x8{};
        }
    };

    f32x16 acc[MT][NT] = {};
    load_w(0, 0);
    load_x(0, 0, fx);
    store_w(0);
    __syncthreads();
    int tap = 0, kb = 0;
    for (int step = 0; step < steps; ++step) {
        const bool more = step + 1 < steps;
        if (++kb == nkb) { kb = 0; ++tap; }
        if (more) {
            load_w(tap, kb);
            load_x(tap, kb, fn);
        }
        const _Float16 *wb = wl[step & 1];
#pragma unroll
        for (int c = 0; c < KB / 16; ++c) {
            f16x8 fw[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                fw[nt] = *reinterpret_cast<const f16x8 *>(wb + (nt * 32 + r) * KB + (((2 * c + h) ^ swz) << 3));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[nt], fx[c][mt], acc[mt][nt], 0, 0, 0);
        }
        if (more) {
            store_w((step + 1) & 1);
#pragma unroll
            for (int c = 0; c < KB / 16; ++c)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) fx[c][mt] = fn[c][mt];
        }
        __syncthreads();
    }
    // register 4j + e of acc[mt][nt] = channel n0 + 32 nt + 8j + 4h + e of pixel m0 + 32 mt + r
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const long p = m0 + mt * 32 + r;
        if (p >= a.M) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = n0 + nt * 32 + 8 * j + 4 * h;
                const size_t o = (size_t)p * a.Cout + co;
                const float4 b = *reinterpret_cast<const float4 *>(a.bias + co);
                float v[4] = {acc[mt][nt][4 * j] + b.x, acc[mt][nt][4 * j + 1] + b.y, acc[mt][nt][4 * j + 2] + b.z,
                              acc[mt][nt][4 * j + 3] + b.w};
                if (a.epi == EPI_RES_RELU) {
                    const f16x4 rs = *reinterpret_cast<const f16x4 *>(a.res + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] + (float)rs[e];
                }
                if (a.epi != EPI_BIAS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                if (a.out_f32) {
                    *reinterpret_cast<float4 *>((float *)a.out + o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    f16x4 ov;
#pragma unroll
                    for (int e = 0; e < 4; ++e) ov[e] = (_Float16)v[e];
                    *reinterpret_cast<f16x4 *>((_Float16 *)a.out + o) = ov;
                }
            }
    }
}

// The tile table: (MT, NT, WM) -> block of (32 MT WM) pixels x (32 NT) channels, largest first.  The wide layers (many pixels)
// take 2 x 2 tiles per wave (four accumulators per operand pair); the deep layers at few frames take one tile per wave in blocks
// of one wave, so that the grid still spreads over the device.  The pick changes no result: an output element's sum is the same
// chain of MFMAs in every tile.
struct Res16Tile { int mt, nt, wm; };
constexpr Res16Tile kTiles[] = {
    {2, 2, 4},    // 0: 256 x 64
    {1, 2, 4},    // 1: 128 x 64
    {1, 2, 2},    // 2: 64 x 64
    {1, 1, 2},    // 3: 64 x 32
    {1, 1, 1},    // 4: 32 x 32
};
constexpr int kNumTiles = (int)(sizeof kTiles / sizeof kTiles[0]);

dim3 res16_grid(int v, long M, int Cout)
{
    const Res16Tile &t = kTiles[v];
    return dim3((unsigned)((M + 32L * t.mt * t.wm - 1) / (32L * t.mt * t.wm)), (unsigned)(Cout / (32 * t.nt)));
}

// the largest tile that still gives every CU a block, else the smallest
int res16_tile_for(long M, int Cout, int num_cus)
{
    const long want = num_cus > 0 ? num_cus : 256;
    for (int v = 0; v < kNumTiles; ++v) {
        const dim3 g = res16_grid(v, M, Cout);
        if ((long)g.x * g.y >= want) return v;
    }
    return kNumTiles - 1;
}

// A tile of one or two accumulators per wave is bound by the latency of a step's loads, not by its MFMAs: it takes steps of 128
// channels where Cin allows, which halves the barriers and doubles the bytes in flight (224^2: 0.39 -> 0.30 ms at 1 frame, 0.63 ->
// 0.54 ms at 32).  The 2 x 2 tile keeps 64: its four accumulators cover the latency, and 128 would leave it one wave per SIMD.
template <int KS>
void launch_res16_conv(int v, dim3 g, hipStream_t st, const Res16Args &a)
{
    const bool wide = a.Cin % 128 == 0;
#define RES16_LAUNCH(MT, NT, WM) \
    do { \
        if (wide) k_res16_conv<MT, NT, WM, KS, 128><<<g, 64 * WM, 0, st>>>(a); \
        else k_res16_conv<MT, NT, WM, KS, 64><<<g, 64 * WM, 0, st>>>(a); \
    } while (0)
    switch (v) {
    case 0: k_res16_conv<2, 2, 4, KS, 64><<<g, 256, 0, st>>>(a); break;
    case 1: RES16_LAUNCH(1, 2, 4); break;
    case 2: RES16_LAUNCH(1, 2, 2); break;
    case 3: RES16_LAUNCH(1, 1, 2); break;
    default: RES16_LAUNCH(1, 1, 1); break;
    }
#undef RES16_LAUNCH
}

struct Res16Layer {                  // one block convolution of the plan
    int cin, cout, k, stride, H, W, Ho, Wo, epi, out_f32;
    _Float16 *w = nullptr;
    float *b = nullptr;
    const _Float16 *in = nullptr, *res = nullptr;
    void *out = nullptr;
};

}  // namespace

struct rva_resnet_f16_plan {
    rva_ctx *ctx = nullptr;
    rva_resnet_desc d{};
    int k = 0;                                             // min(top_k, classes)
    int maps[5][2] = {};                                   // (h, w) of the pooled map and of the four stages
    int tile_force = -1;                                   // RVA_RES16_TILE at creation: every launch takes this tile (tests, tools)
    _Float16 *ws = nullptr, *pooled = nullptr, *mid[N_BLOCKS] = {}, *down[N_BLOCKS] = {}, *outb[N_BLOCKS] = {};
    float *bs = nullptr, *wh = nullptr, *bh = nullptr, *out7 = nullptr, *feat = nullptr;
    Res16Layer conv[N_CONVS];                              // in launch order: per block conv1, [shortcut], conv2
    int n_convs = 0;
    size_t workspace_bytes = 0;
    rva_dev_arena mem;

    // the arena hands out floats: n fp16 elements take (n + 1) / 2 of them
    int alloc_h(_Float16 **dst, size_t n) { return mem.alloc(ctx, reinterpret_cast<float **>(dst), (n + 1) / 2); }
    int upload_h(_Float16 **dst, const std::vector<_Float16> &src)
    {
        const int rc = alloc_h(dst, src.size());
        if (rc != RVA_OK) return rc;
        RVA_HIP(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        return RVA_OK;
    }
};

extern "C" {

int rva_resnet_f16_plan_create(rva_ctx *ctx, const rva_resnet_desc *desc, const rva_resnet_weights *wt, rva_resnet_f16_plan **out)
{
    if (!ctx || !desc || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_f16_plan_create: null argument");
    *out = nullptr;
    const rva_resnet_desc d = *desc;
    if (d.height < 1 || d.width < 1 || d.classes < 1 || d.classes > MAX_CLASSES || d.top_k < 1 || d.max_frames < 1 ||
        d.max_frames > 65535 || (int64_t)d.height * d.width > (1 << 26))
        return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_f16_plan_create: bad descriptor (height, width >= 1, classes 1..%d, top_k >= 1, "
                        "max_frames 1..65535)", MAX_CLASSES);
    bool all = wt->stem_w && wt->stem_b && wt->head_w && wt->head_b;
    for (int i = 0; i < N_CONVS; ++i) all = all && wt->conv[i].w && wt->conv[i].b;
    if (!all) return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_f16_plan_create: every weight array is required");
    auto *p = new rva_resnet_f16_plan();
    p->ctx = ctx;
    p->d = d;
    p->k = std::min(d.top_k, d.classes);
    if (const char *e = getenv("RVA_RES16_TILE")) p->tile_force = std::max(-1, std::min(atoi(e), kNumTiles - 1));
    auto half = [](int n, int k, int pad) { return (n + 2 * pad - k) / 2 + 1; };
    p->maps[0][0] = half(half(d.height, 7, 3), 3, 1);
    p->maps[0][1] = half(half(d.width, 7, 3), 3, 1);
    p->maps[1][0] = p->maps[0][0]; p->maps[1][1] = p->maps[0][1];
    for (int s = 2; s <= 4; ++s) { p->maps[s][0] = half(p->maps[s - 1][0], 3, 1); p->maps[s][1] = half(p->maps[s - 1][1], 3, 1); }
    const size_t mf = (size_t)d.max_frames;
    // sizes first: the workspace must fit before anything is allocated.  fp16 everywhere but out7 and feat.
    size_t act_bytes = mf * p->maps[0][0] * p->maps[0][1] * C_STEM * sizeof(_Float16) + mf * C_FEAT * sizeof(float);
    size_t w_bytes = (size_t)C_STEM * 192 * sizeof(_Float16) + C_STEM * sizeof(float) + (size_t)d.classes * (C_FEAT + 1) * sizeof(float);
    for (int b = 0; b < N_BLOCKS; ++b) {
        const int s = 1 + b / 2, c = C_STEM << (s - 1), cin = (b % 2 == 0 && s > 1) ? c / 2 : c;
        const size_t px = mf * p->maps[s][0] * p->maps[s][1] * c;
        act_bytes += px * (cin != c ? 2 : 1) * sizeof(_Float16) + px * (b == N_BLOCKS - 1 ? sizeof(float) : sizeof(_Float16));
        w_bytes += ((size_t)c * 9 * cin + (size_t)c * 9 * c + (cin != c ? (size_t)c * cin : 0)) * sizeof(_Float16) +
                   (size_t)(cin != c ? 3 : 2) * c * sizeof(float);
    }
    p->workspace_bytes = act_bytes;
    const size_t need = act_bytes + w_bytes;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b) {
        delete p;
        return rva_fail(ctx, RVA_ERR_CAPACITY, "rva_resnet_f16_plan_create: the workspace for %d frames of %d x %d needs %zu MB, the "
                        "device has %zu MB free", d.max_frames, d.height, d.width, need >> 20, free_b >> 20);
    }
    int rc = RVA_OK;
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    std::vector<_Float16> w16;
    char bad[24] = "";
    // rounds one array and uploads it as it is ([Cout][k*k][Cin] is what the kernel reads); names the array that fails
    auto upload_w = [&](_Float16 **dst, const float *src, size_t n, const char *name, int idx) {
        if (rc != RVA_OK) return;
        if (!rva_round_f16(src, n, w16)) {
            if (idx >= 0) snprintf(bad, sizeof bad, "conv[%d].w", idx);
            else snprintf(bad, sizeof bad, "%s", name);
            rc = RVA_ERR_ARG;
            return;
        }
        rc = p->upload_h(dst, w16);
    };
    if (!rva_round_f16(wt->stem_w, (size_t)C_STEM * 147, w16)) { snprintf(bad, sizeof bad, "stem_w"); rc = RVA_ERR_ARG; }
    else step(p->upload_h(&p->ws, rva_clip16_stem_pack(w16)));
    step(p->mem.upload(ctx, &p->bs, wt->stem_b, C_STEM));
    step(p->mem.upload(ctx, &p->wh, wt->head_w, (size_t)d.classes * C_FEAT));
    step(p->mem.upload(ctx, &p->bh, wt->head_b, d.classes));
    step(p->alloc_h(&p->pooled, mf * p->maps[0][0] * p->maps[0][1] * C_STEM));
    step(p->mem.alloc(ctx, &p->feat, mf * C_FEAT));
    const _Float16 *x = p->pooled;
    int wi = 0, hin = p->maps[0][0], win = p->maps[0][1];
    for (int b = 0; b < N_BLOCKS; ++b) {
        const int s = 1 + b / 2, c = C_STEM << (s - 1), cin = (b % 2 == 0 && s > 1) ? c / 2 : c, stride = cin != c ? 2 : 1;
        const int ho = p->maps[s][0], wo = p->maps[s][1];
        const size_t px = mf * ho * wo * c;
        const bool last = b == N_BLOCKS - 1;
        step(p->alloc_h(&p->mid[b], px));
        if (last) step(p->mem.alloc(ctx, &p->out7, px));
        else step(p->alloc_h(&p->outb[b], px));
        if (cin != c) step(p->alloc_h(&p->down[b], px));
        // the ABI's weight order of a block: conv1, conv2, then the shortcut
        _Float16 *w1 = nullptr, *w2 = nullptr, *wd = nullptr;
        float *b1 = nullptr, *b2 = nullptr, *bd = nullptr;
        upload_w(&w1, wt->conv[wi].w, (size_t)c * 9 * cin, nullptr, wi);
        step(p->mem.upload(ctx, &b1, wt->conv[wi].b, c));
        upload_w(&w2, wt->conv[wi + 1].w, (size_t)c * 9 * c, nullptr, wi + 1);
        step(p->mem.upload(ctx, &b2, wt->conv[wi + 1].b, c));
        wi += 2;
        if (cin != c) {
            upload_w(&wd, wt->conv[wi].w, (size_t)c * cin, nullptr, wi);
            step(p->mem.upload(ctx, &bd, wt->conv[wi].b, c));
            ++wi;
        }
        Res16Layer l1{cin, c, 3, stride, hin, win, ho, wo, EPI_RELU, 0};
        l1.w = w1; l1.b = b1; l1.in = x; l1.out = p->mid[b];
        p->conv[p->n_convs++] = l1;
        if (cin != c) {
            Res16Layer ld{cin, c, 1, 2, hin, win, ho, wo, EPI_BIAS, 0};
            ld.w = wd; ld.b = bd; ld.in = x; ld.out = p->down[b];
            p->conv[p->n_convs++] = ld;
        }
        Res16Layer l2{c, c, 3, 1, ho, wo, ho, wo, EPI_RES_RELU, last ? 1 : 0};
        l2.w = w2; l2.b = b2; l2.in = p->mid[b]; l2.res = cin != c ? p->down[b] : x;
        l2.out = last ? (void *)p->out7 : (void *)p->outb[b];
        p->conv[p->n_convs++] = l2;
        x = p->outb[b];
        hin = ho; win = wo;
    }
    if (rc == RVA_OK) rc = rva_clip16_stem_prepare(ctx);
    if (rc == RVA_OK) rc = rva_clip_head_prepare(ctx, C_FEAT);
    if (rc == RVA_OK) rc = rva_clip_post_prepare(ctx, d.classes);
    if (rc != RVA_OK) {
        rva_resnet_f16_plan_destroy(p);
        if (bad[0]) return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_f16_plan_create: a value of %s does not stay finite in fp16", bad);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

void rva_resnet_f16_plan_destroy(rva_resnet_f16_plan *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

int rva_resnet_f16_plan_info(const rva_resnet_f16_plan *p, int32_t *maps, int64_t *workspace_bytes, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    if (maps)
        for (int s = 0; s < 5; ++s) { maps[2 * s] = p->maps[s][0]; maps[2 * s + 1] = p->maps[s][1]; }
    if (workspace_bytes) *workspace_bytes = (int64_t)p->workspace_bytes;
    if (n_launches) *n_launches = 1 + N_CONVS + 2;
    return RVA_OK;
}

int rva_resnet_f16_plan_run(rva_resnet_f16_plan *p, const void *frames, const int32_t *frame_index, int n, void *logits, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n < 1 || n > p->d.max_frames)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_f16_plan_run: bad argument (n %d, capacity %d)", n, p->d.max_frames);
    const hipStream_t st = (hipStream_t)stream_;
    int rc = rva_clip16_stem_launch(ctx, (const _Float16 *)frames, frame_index, p->ws, p->bs, p->pooled, p->d.height, p->d.width, n, st);
    if (rc != RVA_OK) return rc;
    const int cus = rva_num_cus(ctx);
    for (int i = 0; i < p->n_convs; ++i) {
        const Res16Layer &l = p->conv[i];
        Res16Args a{};
        a.in = l.in; a.w = l.w; a.bias = l.b; a.res = l.res; a.out = l.out;
        a.H = l.H; a.W = l.W; a.Ho = l.Ho; a.Wo = l.Wo; a.Cin = l.cin; a.Cout = l.cout; a.stride = l.stride; a.epi = l.epi;
        a.out_f32 = l.out_f32;
        a.M = (long)n * l.Ho * l.Wo;
        const int v = p->tile_force >= 0 ? p->tile_force : res16_tile_for(a.M, l.cout, cus);
        const dim3 g = res16_grid(v, a.M, l.cout);
        if (l.k == 3) launch_res16_conv<3>(v, g, st, a);
        else launch_res16_conv<1>(v, g, st, a);
        RVA_HIP(ctx, hipGetLastError());
    }
    rc = rva_res_mean_launch(ctx, p->out7, p->maps[4][0] * p->maps[4][1], p->feat, n, st);
    if (rc != RVA_OK) return rc;
    return rva_clip_head_launch(ctx, p->feat, p->wh, p->bh, (float *)logits, C_FEAT, p->d.classes, n, st);
}

int rva_resnet_f16_plan_run_post(rva_resnet_f16_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                                 void *cls, void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, "rva_resnet_f16_plan_run_post", (const float *)logits, p->d.classes, p->k, rows, n_rows, max_det,
                                (float *)scores, (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  Every tensor is frame-major NHWC; the
// counts are ELEMENT counts of the stage's stored type (fp16 for every stage but OUT0 + 7 and FEAT).
int rva_resnet_f16_plan_stage(rva_resnet_f16_plan *p, int stage, int n, void *dst, int64_t dst_elems, int64_t *n_elems, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (n < 1 || n > p->d.max_frames)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_f16_plan_stage: bad argument (n %d, capacity %d)", n, p->d.max_frames);
    const void *src = nullptr;
    int64_t count = 0;
    size_t elem = sizeof(_Float16);
    auto block = [&](_Float16 *const *bufs, int b) {
        const int s = 1 + b / 2;
        src = bufs[b];
        count = (int64_t)n * p->maps[s][0] * p->maps[s][1] * (C_STEM << (s - 1));
    };
    if (stage == RVA_RESNET_STAGE_POOLED) { src = p->pooled; count = (int64_t)n * p->maps[0][0] * p->maps[0][1] * C_STEM; }
    else if (stage >= RVA_RESNET_STAGE_MID0 && stage < RVA_RESNET_STAGE_MID0 + N_BLOCKS) block(p->mid, stage - RVA_RESNET_STAGE_MID0);
    else if (stage >= RVA_RESNET_STAGE_DOWN2 && stage <= RVA_RESNET_STAGE_DOWN6) block(p->down, 2 * (stage - RVA_RESNET_STAGE_DOWN2) + 2);
    else if (stage >= RVA_RESNET_STAGE_OUT0 && stage < RVA_RESNET_STAGE_OUT0 + N_BLOCKS) {
        block(p->outb, stage - RVA_RESNET_STAGE_OUT0);
        if (stage == RVA_RESNET_STAGE_OUT0 + N_BLOCKS - 1) { src = p->out7; elem = sizeof(float); }
    }
    else if (stage == RVA_RESNET_STAGE_FEAT) { src = p->feat; count = (int64_t)n * C_FEAT; elem = sizeof(float); }
    else return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_f16_plan_stage: unknown stage %d", stage);
    if (n_elems) *n_elems = count;
    if (!dst) return RVA_OK;
    if (dst_elems < count)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_resnet_f16_plan_stage: dst holds %lld elements, stage %d of %d frames has %lld",
                        (long long)dst_elems, stage, n, (long long)count);
    RVA_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)count * elem, hipMemcpyDeviceToDevice, (hipStream_t)stream_));
    return RVA_OK;
}

}  // extern "C"
