// The ResNet classifiers for `half: true` (engine "resnet-f16"): ONE plan that walks rva_res_topology (rva_plan_topo.h: any ResNet
// of the torchvision family, BasicBlocks or Bottlenecks, 1..64 blocks per stage) with fp16 frames, fp16 convolution weights and
// fp16 stored activations, and every sum in fp32.  It has two front doors: rva_resnet_f16_plan_* (the ResNet-18 of rva_resnet.hip:
// its descriptor, weights struct, stage codes and texts, mapped by rva_res18_desc / rva_res18_stage onto BasicBlocks 2, 2, 2, 2
// with split shortcuts -- the same launches and taps as the fp32 plan) and rva_resnetx_f16_plan_* (any depth).  Below, the stage
// names and counts are ResNet-18's (19 convolutions, mid0..7, down2/4/6, out0..7; "out7" = the last block's output in general).
// The numeric contract is that of clip-f16 / clip3d-f16:
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
//   K_mean / K_head / K_post: k_res_mean through rva_res_mean_launch (rva_resnet.hip; 512 or 2048 channels) and the head and top-k
//            kernels of rva_clip.hip, unchanged.
//
// Every stage keeps its own workspace buffer (the _stage entries read them).
//
// One piece of device code serves only plans without RVA_RESX_SPLIT_SHORTCUT (never ResNet-18's entries):
//
//   K_conv, DUAL   a block that has a shortcut convolution computes ReLU(conv_close(mid) + b_close + conv_short(x) + b_short): as a
//            GEMM, one accumulator chain over [taps of conv_close | channels of x].  k_res16_conv<..., DUAL = true> runs, after the
//            TAPS * Cin / KB steps of the closing convolution, Cin2 / KB further steps whose activation operand is x at (y * s2,
//            x * s2) of its own H2 x W2 map (1x1, pad 0: always in range; create checks Ho == (H2 - 1) / s2 + 1) and whose weights
//            come from the shortcut's [Cout][Cin2] array through the same LDS double buffer and swizzle.  Steps of 128 channels only
//            where both Cin and Cin2 allow them; the 16-channel chunks run in the same order for either step, so tile and step still
//            change no bit.  The bias is b_close + b_short (added in float64 by the packer, rounded once), the epilogue EPI_RELU.
//            One launch, one fp16 rounding and the write and re-read of the `down` tensor fewer per such block.  A plan created with
//            RVA_RESX_SPLIT_SHORTCUT launches the shortcut on its own (EPI_BIAS) and adds it as the residual (EPI_RES_RELU): the
//            launches and bits of the ResNet-18 entries.
#include "rva_mfma_f16.h"
#include "rva_plan_topo.h"

namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct Res16Args {
    const _Float16 *in;              // [n][H][W][Cin]
    const _Float16 *w;               // [Cout][KS*KS][Cin]
    const float *bias;               // [Cout]
    const _Float16 *res;             // [n][Ho][Wo][Cout] (EPI_RES_RELU)
    void *out;                       // [n][Ho][Wo][Cout], fp16 or (out_f32) fp32
    int H, W, Ho, Wo, Cin, Cout, stride, epi, out_f32;
    long M;                          // n * Ho * Wo
    // DUAL only: the block's shortcut convolution (1x1, pad 0) as further steps of the same sum
    const _Float16 *in2;             // [n][H2][W2][Cin2], read at (y * stride2, x * stride2) of output pixel (y, x)
    const _Float16 *w2;              // [Cout][Cin2]
    int H2, W2, Cin2, stride2;
};

// ---------------------------------------------------------------------------------------------------
// K_conv.  A wave owns MT tiles of 32 pixels x NT tiles of 32 channels; the WM waves of a block share the 32 NT channels (their
// weights go through LDS once per block) and take consecutive runs of 32 MT pixels: block = 32 MT WM pixels x 32 NT channels.
// A step is KB = 64 or 128 input channels (four or eight MFMA chunks); Cin is a multiple of KB and Cout of 32 NT: no K tail and no
// channel tail.  The chunks run in the same order for either KB.
// DUAL: after the TAPS * Cin / KB steps of the convolution itself, Cin2 / KB further steps of the block's shortcut convolution on
// the block's input -- one accumulator chain over [taps of w | channels of in2], the weights of the further steps through the same
// LDS double buffer and swizzle.  Cin2 is a multiple of KB too.
template <int MT, int NT, int WM, int KS, int KB, bool DUAL = false>
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
    const int nkb = a.Cin / KB, steps1 = TAPS * nkb;
    int steps = steps1;
    if constexpr (DUAL) steps += a.Cin2 / KB;

    int py[MT], px[MT];
    size_t pimg[MT];
    [[maybe_unused]] size_t p2[MT];                          // DUAL: the pixel of in2 a column reads
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        long p = m0 + mt * 32 + r;
        pv[mt] = p < a.M;
        if (!pv[mt]) p = 0;
        px[mt] = (int)(p % a.Wo) * a.stride - PAD;
        py[mt] = (int)((p / a.Wo) % a.Ho) * a.stride - PAD;
        pimg[mt] = (size_t)(p / ((long)a.Wo * a.Ho)) * a.H * a.W;
        if constexpr (DUAL)
            p2[mt] = ((size_t)(p / ((long)a.Wo * a.Ho)) * a.H2 + (size_t)((p / a.Wo) % a.Ho) * a.stride2) * a.W2 +
                     (size_t)(p % a.Wo) * a.stride2;
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

    // DUAL: step steps1 + k2 = channels k2 * KB .. of the shortcut convolution, always in range (1x1, pad 0)
    [[maybe_unused]] auto load_w2 = [&](int k2) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int s = tid + THREADS * j, row = s / (KB / 8), q = s % (KB / 8);
            st[j] = *reinterpret_cast<const f16x8 *>(a.w2 + (size_t)(n0 + row) * a.Cin2 + k2 * KB + q * 8);
        }
    };
    [[maybe_unused]] auto load_x2 = [&](int k2, f16x8 (&f)[KB / 16][MT]) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const _Float16 *arow = a.in2 + (pv[mt] ? p2[mt] : 0) * a.Cin2 + k2 * KB + 8 * h;
#pragma unroll
            for (int c = 0; c < KB / 16; ++c) f[c][mt] = pv[mt] ? *reinterpret_cast<const f16x8 *>(arow + 16 * c) : f16x8{};
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
            if constexpr (DUAL) {
                if (step + 1 >= steps1) {
                    load_w2(step + 1 - steps1);
                    load_x2(step + 1 - steps1, fn);
                } else {
                    load_w(tap, kb);
                    load_x(tap, kb, fn);
                }
            } else {
                load_w(tap, kb);
                load_x(tap, kb, fn);
            }
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

// The same table for a closing convolution that carries its block's shortcut convolution (DUAL): steps of 128 channels only where
// both Cin and Cin2 allow them.
template <int KS>
void launch_res16_dual(int v, dim3 g, hipStream_t st, const Res16Args &a)
{
    const bool wide = a.Cin % 128 == 0 && a.Cin2 % 128 == 0;
#define RES16_LAUNCH(MT, NT, WM) \
    do { \
        if (wide) k_res16_conv<MT, NT, WM, KS, 128, true><<<g, 64 * WM, 0, st>>>(a); \
        else k_res16_conv<MT, NT, WM, KS, 64, true><<<g, 64 * WM, 0, st>>>(a); \
    } while (0)
    switch (v) {
    case 0: k_res16_conv<2, 2, 4, KS, 64, true><<<g, 256, 0, st>>>(a); break;
    case 1: RES16_LAUNCH(1, 2, 4); break;
    case 2: RES16_LAUNCH(1, 2, 2); break;
    case 3: RES16_LAUNCH(1, 1, 2); break;
    default: RES16_LAUNCH(1, 1, 1); break;
    }
#undef RES16_LAUNCH
}

}  // namespace

// The one plan of this file.  rva_resnet_f16_plan (ResNet-18) is the same object under its own handle type: created with
// rva_res18_desc, tapped through rva_res18_stage.
struct rva_resnetx_f16_plan {
    rva_ctx *ctx = nullptr;
    rva_resnetx_desc d{};
    int k = 0;                                             // min(top_k, classes)
    rva_res_topo t;
    int tile_force = -1;                                   // RVA_RES16_TILE at creation: every launch takes this tile (tests, tools)
    _Float16 *ws = nullptr;
    float *bs = nullptr, *wh = nullptr, *bh = nullptr;
    std::vector<_Float16 *> w;                             // of convs[i], in the ABI's order
    std::vector<float *> b;
    std::vector<void *> stage;                             // indexed by stage code; null: the plan has no such stage
    size_t workspace_bytes = 0;
    rva_dev_arena mem;
    // every stage is stored as fp16 but the last block's output (it feeds only the mean) and feat
    size_t esize(int s) const { return s == t.last_out || s == RVA_RESX_FEAT ? sizeof(float) : sizeof(_Float16); }
};

namespace {

typedef rva_resnetx_f16_plan Plan;
Plan *plan_of(rva_resnet_f16_plan *p) { return reinterpret_cast<Plan *>(p); }
const Plan *plan_of(const rva_resnet_f16_plan *p) { return reinterpret_cast<const Plan *>(p); }

void res16_destroy(Plan *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

// a create after the entry's own argument checks: d, t = rva_res_topology(d) and every array of wt are good
int res16_create(rva_ctx *ctx, const char *who, const rva_resnetx_desc &d, const rva_res_topo &t, const rva_resnetx_weights &wt, Plan **out)
{
    for (const rva_res_conv &c : t.conv) {                 // what the kernel takes; holds for every net of the family
        const bool dual = c.in2 >= 0;
        if (c.cin % 64 || c.cout % 64 || (dual && (c.cin2 % 64 || c.Ho != (c.H2 - 1) / c.stride2 + 1 || c.Wo != (c.W2 - 1) / c.stride2 + 1)))
            return rva_fail(ctx, RVA_ERR_ARG, "%s: a convolution of %d -> %d channels does not fit the kernel", who, c.cin, c.cout);
    }
    auto *p = new Plan();
    p->ctx = ctx;
    p->d = d;
    p->k = std::min(d.top_k, d.classes);
    p->t = t;
    const size_t mf = (size_t)d.max_frames;
    // sizes first: the workspace must fit before anything is allocated
    size_t act_bytes = 0;
    size_t w_bytes = (size_t)RES_C_STEM * 192 * sizeof(_Float16) + RES_C_STEM * sizeof(float) + (size_t)d.classes * (t.c_feat + 1) * sizeof(float);
    for (size_t s = 0; s < t.elems.size(); ++s) act_bytes += mf * t.elems[s] * p->esize((int)s);
    for (int i = 0; i < t.n_convs; ++i) w_bytes += t.conv_weights[i] * sizeof(_Float16) + t.conv_cout[i] * sizeof(float);
    char shape[64];
    snprintf(shape, sizeof shape, "%d frames of %d x %d", d.max_frames, d.height, d.width);
    int rc = rva_plan_fits(ctx, who, act_bytes + w_bytes, shape);
    if (rc != RVA_OK) {
        res16_destroy(p);                                  // nothing on the device yet
        return rc;
    }
    p->workspace_bytes = act_bytes;
    p->w.assign(t.n_convs, nullptr);
    p->b.assign(t.n_convs, nullptr);
    p->stage.assign(t.elems.size(), nullptr);
    if (const char *e = getenv("RVA_RES16_TILE")) p->tile_force = std::max(-1, std::min(atoi(e), kNumTiles - 1));
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    std::vector<_Float16> w16;
    char bad[24] = "";
    if (!rva_round_f16(wt.stem_w, (size_t)RES_C_STEM * 147, w16)) { snprintf(bad, sizeof bad, "stem_w"); rc = RVA_ERR_ARG; }
    else { w16 = rva_clip16_stem_pack(w16); step(p->mem.upload(ctx, &p->ws, w16.data(), w16.size())); }
    step(p->mem.upload(ctx, &p->bs, wt.stem_b, RES_C_STEM));
    step(p->mem.upload(ctx, &p->wh, wt.head_w, (size_t)d.classes * t.c_feat));
    step(p->mem.upload(ctx, &p->bh, wt.head_b, d.classes));
    for (size_t s = 0; s < t.elems.size(); ++s) {
        if (!t.elems[s]) continue;
        char *m = nullptr;
        step(p->mem.alloc(ctx, &m, mf * t.elems[s] * p->esize((int)s)));
        p->stage[s] = m;
    }
    // in the ABI's weight order: rounds an array and uploads it as it is ([Cout][k*k][Cin] is what the kernel reads); names the
    // first array that fails
    for (int i = 0; i < t.n_convs && rc == RVA_OK; ++i) {
        if (!rva_round_f16(wt.convs[i].w, t.conv_weights[i], w16)) {
            snprintf(bad, sizeof bad, "conv[%d].w", i);
            rc = RVA_ERR_ARG;
            break;
        }
        step(p->mem.upload(ctx, &p->w[i], w16.data(), w16.size()));
        step(p->mem.upload(ctx, &p->b[i], wt.convs[i].b, t.conv_cout[i]));
    }
    if (rc == RVA_OK) rc = rva_clip16_stem_prepare(ctx);
    if (rc == RVA_OK) rc = rva_clip_head_prepare(ctx, t.c_feat);
    if (rc == RVA_OK) rc = rva_clip_post_prepare(ctx, d.classes);
    if (rc != RVA_OK) {
        res16_destroy(p);
        if (bad[0]) return rva_fail(ctx, RVA_ERR_ARG, "%s: a value of %s does not stay finite in fp16", who, bad);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

int res16_run(Plan *p, const char *who, const void *frames, const int32_t *frame_index, int n, void *logits, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n < 1 || n > p->d.max_frames)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad argument (n %d, capacity %d)", who, n, p->d.max_frames);
    const hipStream_t st = (hipStream_t)stream_;
    void *const *buf = p->stage.data();
    int rc = rva_clip16_stem_launch(ctx, (const _Float16 *)frames, frame_index, p->ws, p->bs, (_Float16 *)buf[RVA_RESX_POOLED], p->d.height,
                                    p->d.width, n, st);
    if (rc != RVA_OK) return rc;
    const int cus = rva_num_cus(ctx);
    for (const rva_res_conv &l : p->t.conv) {
        Res16Args a{};
        a.in = (const _Float16 *)buf[l.in]; a.w = p->w[l.wi]; a.bias = p->b[l.wi]; a.out = buf[l.out];
        a.res = l.res >= 0 ? (const _Float16 *)buf[l.res] : nullptr;
        a.H = l.H; a.W = l.W; a.Ho = l.Ho; a.Wo = l.Wo; a.Cin = l.cin; a.Cout = l.cout; a.stride = l.stride; a.epi = l.epi;
        a.out_f32 = l.out == p->t.last_out;
        a.M = (long)n * l.Ho * l.Wo;
        const int v = p->tile_force >= 0 ? p->tile_force : res16_tile_for(a.M, l.cout, cus);
        const dim3 g = res16_grid(v, a.M, l.cout);
        if (l.in2 >= 0) {
            a.in2 = (const _Float16 *)buf[l.in2]; a.w2 = p->w[l.wi2];
            a.H2 = l.H2; a.W2 = l.W2; a.Cin2 = l.cin2; a.stride2 = l.stride2;
            if (l.k == 3) launch_res16_dual<3>(v, g, st, a);
            else launch_res16_dual<1>(v, g, st, a);
        } else if (l.k == 3) {
            launch_res16_conv<3>(v, g, st, a);
        } else {
            launch_res16_conv<1>(v, g, st, a);
        }
        RVA_HIP(ctx, hipGetLastError());
    }
    float *feat = (float *)buf[RVA_RESX_FEAT];
    rc = rva_res_mean_launch(ctx, (const float *)buf[p->t.last_out], p->t.maps[4][0] * p->t.maps[4][1], p->t.c_feat, feat, n, st);
    if (rc != RVA_OK) return rc;
    return rva_clip_head_launch(ctx, feat, p->wh, p->bh, (float *)logits, p->t.c_feat, p->d.classes, n, st);
}

int res16_run_post(Plan *p, const char *who, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores, void *cls,
                   void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, who, (const float *)logits, p->d.classes, p->k, rows, n_rows, max_det, (float *)scores,
                                (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

int res16_info(const Plan *p, int32_t *maps, int64_t *workspace_bytes, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    rva_res_info(p->t, p->workspace_bytes, maps, workspace_bytes, n_launches);
    return RVA_OK;
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  Every tensor is frame-major NHWC; the
// counts are ELEMENT counts of the stage's stored type.  `stage` is the plan's code of what the entry's caller named `asked`.
int res16_stage(Plan *p, const char *who, int asked, int stage, int n, void *dst, int64_t dst_elems, int64_t *n_elems, rva_stream_t stream_)
{
    rva_ctx *ctx = p->ctx;
    if (n < 1 || n > p->d.max_frames) return rva_fail(ctx, RVA_ERR_ARG, "%s: bad argument (n %d, capacity %d)", who, n, p->d.max_frames);
    if (stage < 0 || stage >= (int)p->stage.size() || !p->stage[stage])
        return rva_fail(ctx, RVA_ERR_ARG, "%s: the plan has no stage %d", who, asked);
    return rva_clip_stage_copy(ctx, who, asked, n, "frames", p->stage[stage], p->esize(stage), "elements", n * p->t.elems[stage], 0, 0, 0,
                               dst, dst_elems, n_elems, (hipStream_t)stream_);
}

}  // namespace

extern "C" {

// ResNet-18: the checks and texts of its own entries, then the plan of BasicBlocks 2, 2, 2, 2 with split shortcuts.
int rva_resnet_f16_plan_create(rva_ctx *ctx, const rva_resnet_desc *desc, const rva_resnet_weights *wt, rva_resnet_f16_plan **out)
{
    const char *who = "rva_resnet_f16_plan_create";
    const int rc = rva_res_check_args(ctx, who, desc, wt, (void **)out);
    if (rc != RVA_OK) return rc;
    const rva_resnetx_desc d = rva_res18_desc(*desc);
    return res16_create(ctx, who, d, rva_res_topology(d), {wt->stem_w, wt->stem_b, wt->conv, wt->head_w, wt->head_b}, (Plan **)out);
}

void rva_resnet_f16_plan_destroy(rva_resnet_f16_plan *p) { res16_destroy(plan_of(p)); }

int rva_resnet_f16_plan_info(const rva_resnet_f16_plan *p, int32_t *maps, int64_t *workspace_bytes, int32_t *n_launches)
{
    return res16_info(plan_of(p), maps, workspace_bytes, n_launches);
}

int rva_resnet_f16_plan_run(rva_resnet_f16_plan *p, const void *frames, const int32_t *frame_index, int n, void *logits, rva_stream_t stream)
{
    return res16_run(plan_of(p), "rva_resnet_f16_plan_run", frames, frame_index, n, logits, stream);
}

int rva_resnet_f16_plan_run_post(rva_resnet_f16_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                                 void *cls, void *boxes, void *counts, rva_stream_t stream)
{
    return res16_run_post(plan_of(p), "rva_resnet_f16_plan_run_post", logits, rows, n_rows, max_det, scores, cls, boxes, counts, stream);
}

// the tap by RVA_RESNET_STAGE_* code: fp16 elements for every stage but OUT0 + 7 and FEAT
int rva_resnet_f16_plan_stage(rva_resnet_f16_plan *p, int stage, int n, void *dst, int64_t dst_elems, int64_t *n_elems, rva_stream_t stream)
{
    if (!p) return RVA_ERR_ARG;
    const char *who = "rva_resnet_f16_plan_stage";
    const int code = rva_res18_stage(stage);
    if (code < 0) return rva_fail(plan_of(p)->ctx, RVA_ERR_ARG, "%s: unknown stage %d", who, stage);
    return res16_stage(plan_of(p), who, stage, code, n, dst, dst_elems, n_elems, stream);
}

// Any ResNet of the family: a block's shortcut convolution runs inside its closing convolution's launch (DUAL) unless the plan
// was created with RVA_RESX_SPLIT_SHORTCUT.
int rva_resnetx_f16_plan_create(rva_ctx *ctx, const rva_resnetx_desc *desc, const rva_resnetx_weights *wt, rva_resnetx_f16_plan **out)
{
    const char *who = "rva_resnetx_f16_plan_create";
    if (!ctx || !desc || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    const rva_resnetx_desc d = *desc;
    bool ok = d.height >= 1 && d.width >= 1 && d.classes >= 1 && d.classes <= RVA_PLAN_MAX_CLASSES && d.top_k >= 1 && d.max_frames >= 1 &&
              d.max_frames <= 65535 && (int64_t)d.height * d.width <= (1 << 26) && (d.bottleneck == 0 || d.bottleneck == 1) &&
              (d.flags & ~RVA_RESX_SPLIT_SHORTCUT) == 0;
    for (int s = 0; s < 4; ++s) ok = ok && d.blocks[s] >= 1 && d.blocks[s] <= 64;
    if (!ok)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad descriptor (height, width >= 1, classes 1..%d, top_k >= 1, max_frames 1..65535, "
                        "bottleneck 0 or 1, blocks 1..64 each, flags 0 or RVA_RESX_SPLIT_SHORTCUT)", who, RVA_PLAN_MAX_CLASSES);
    const rva_res_topo t = rva_res_topology(d);
    if (d.n_convs != t.n_convs)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad descriptor (n_convs %d, the topology has %d convolutions)", who, d.n_convs, t.n_convs);
    bool all = wt->stem_w && wt->stem_b && wt->head_w && wt->head_b && wt->convs;
    for (int i = 0; all && i < t.n_convs; ++i) all = wt->convs[i].w && wt->convs[i].b;
    if (!all) return rva_fail(ctx, RVA_ERR_ARG, "%s: every weight array is required", who);
    return res16_create(ctx, who, d, t, *wt, out);
}

void rva_resnetx_f16_plan_destroy(rva_resnetx_f16_plan *p) { res16_destroy(p); }

int rva_resnetx_f16_plan_info(const rva_resnetx_f16_plan *p, int32_t *maps, int64_t *workspace_bytes, int32_t *n_launches)
{
    return res16_info(p, maps, workspace_bytes, n_launches);
}

int rva_resnetx_f16_plan_run(rva_resnetx_f16_plan *p, const void *frames, const int32_t *frame_index, int n, void *logits, rva_stream_t stream)
{
    return res16_run(p, "rva_resnetx_f16_plan_run", frames, frame_index, n, logits, stream);
}

int rva_resnetx_f16_plan_run_post(rva_resnetx_f16_plan *p, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores,
                                  void *cls, void *boxes, void *counts, rva_stream_t stream)
{
    return res16_run_post(p, "rva_resnetx_f16_plan_run_post", logits, rows, n_rows, max_det, scores, cls, boxes, counts, stream);
}

// the tap by RVA_RESX_* code; a stage code the plan has no buffer for is refused
int rva_resnetx_f16_plan_stage(rva_resnetx_f16_plan *p, int stage, int n, void *dst, int64_t dst_elems, int64_t *n_elems, rva_stream_t stream)
{
    if (!p) return RVA_ERR_ARG;
    return res16_stage(p, "rva_resnetx_f16_plan_stage", stage, stage, n, dst, dst_elems, n_elems, stream);
}

}  // extern "C"

