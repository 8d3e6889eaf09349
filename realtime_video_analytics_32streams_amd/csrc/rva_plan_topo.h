// Host-only descriptions of the networks that exist as an fp32 and an fp16 plan: the shapes, the order of the launches, what each
// launch reads and writes, the argument checks, _info and the stage -> element count resolution.  The plan files walk these and add
// what differs by precision (element sizes, rounding, kernels).  Nothing here is device code.
#pragma once

#include "rva_internal.h"

// ---------------------------------------------------------------------------------------------------
// ResNet (rva_resnet.hip: fp32 ResNet-18; rva_resnet_f16.hip: fp16, any depth): ONE topology, that of any ResNet of the torchvision
// family -- the stem, then four stages of blocks[s] BasicBlocks or Bottlenecks (expansion 4, stride on the 3x3) of width 64 << s; a
// block whose stride is not 1 or whose input width differs from its output width has a 1x1 shortcut convolution.  Stage codes:
// RVA_RESX_POOLED, RVA_RESX_FEAT, RVA_RESX_BLOCK0 + 4 b + slot.  ResNet-18 is a case of it (rva_res18_desc, rva_res18_stage below).
constexpr int RES_C_STEM = 64, RES_C_FEAT = 512;
constexpr int RES_CONVS = 19;                                   // of rva_resnet_weights::conv (ResNet-18)
constexpr int EPI_RELU = 0, EPI_BIAS = 1, EPI_RES_RELU = 2;     // max(acc + b, 0) | acc + b | max((acc + b) + res, 0)

struct rva_res_conv {                // one launch
    int cin, cout, k, stride, H, W, Ho, Wo, epi;
    int in, res, out;                // the stage codes it reads, adds as residual (-1: none) and writes
    int wi;                          // its index in rva_resnetx_weights::convs
    int in2, wi2, cin2, stride2, H2, W2;   // in2 >= 0: the shortcut convolution convs[wi2] runs inside this launch, on stage in2
    size_t weights() const { return (size_t)cout * k * k * cin; }
};

struct rva_res_topo {
    int maps[5][2];                  // (h, w) of the pooled map and of the four stages
    int c_feat = 0, n_blocks = 0, n_convs = 0, last_out = 0;
    std::vector<rva_res_conv> conv;  // in launch order
    std::vector<size_t> conv_weights;  // of convs[i], in the ABI's order
    std::vector<int> conv_cout;
    std::vector<int64_t> elems;      // elements of a stage per frame; 0: the plan has no such stage
};

inline rva_res_topo rva_res_topology(const rva_resnetx_desc &d)
{
    rva_res_topo t;
    int hc, wc;
    rva_stem_maps(d.height, d.width, &hc, &wc, &t.maps[0][0], &t.maps[0][1]);
    t.maps[1][0] = t.maps[0][0]; t.maps[1][1] = t.maps[0][1];
    for (int s = 2; s <= 4; ++s) { t.maps[s][0] = rva_half_map(t.maps[s - 1][0], 3, 1); t.maps[s][1] = rva_half_map(t.maps[s - 1][1], 3, 1); }
    const bool bott = d.bottleneck != 0, split = (d.flags & RVA_RESX_SPLIT_SHORTCUT) != 0;
    const int exp = bott ? 4 : 1;
    t.n_blocks = d.blocks[0] + d.blocks[1] + d.blocks[2] + d.blocks[3];
    t.c_feat = RES_C_FEAT * exp;
    t.elems.assign(RVA_RESX_BLOCK0 + 4 * (size_t)t.n_blocks, 0);
    t.elems[RVA_RESX_POOLED] = (int64_t)t.maps[0][0] * t.maps[0][1] * RES_C_STEM;
    t.elems[RVA_RESX_FEAT] = t.c_feat;
    int x = RVA_RESX_POOLED, cin = RES_C_STEM, wi = 0, b = 0, hin = t.maps[0][0], win = t.maps[0][1];
    auto weights = [&](int co, int k, int ci) { t.conv_weights.push_back((size_t)co * k * k * ci); t.conv_cout.push_back(co); };
    for (int s = 0; s < 4; ++s)
        for (int j = 0; j < d.blocks[s]; ++j, ++b) {
            const int width = RES_C_STEM << s, cout = width * exp, stride = (j == 0 && s > 0) ? 2 : 1;
            const bool shortcut = stride != 1 || cin != cout;
            const int ho = t.maps[1 + s][0], wo = t.maps[1 + s][1];
            const int base = RVA_RESX_BLOCK0 + 4 * b, mid1 = base, mid2 = base + 1, down = base + 2, out = base + 3;
            const int n_own = bott ? 3 : 2, wi_short = wi + n_own;
            int close_in, close_cin, close_k;
            if (bott) {
                t.elems[mid1] = (int64_t)hin * win * width;
                t.elems[mid2] = (int64_t)ho * wo * width;
                t.conv.push_back({cin, width, 1, 1, hin, win, hin, win, EPI_RELU, x, -1, mid1, wi, -1, -1, 0, 0, 0, 0});
                t.conv.push_back({width, width, 3, stride, hin, win, ho, wo, EPI_RELU, mid1, -1, mid2, wi + 1, -1, -1, 0, 0, 0, 0});
                weights(width, 1, cin); weights(width, 3, width); weights(cout, 1, width);
                close_in = mid2; close_cin = width; close_k = 1;
            } else {
                t.elems[mid1] = (int64_t)ho * wo * width;
                t.conv.push_back({cin, width, 3, stride, hin, win, ho, wo, EPI_RELU, x, -1, mid1, wi, -1, -1, 0, 0, 0, 0});
                weights(width, 3, cin); weights(cout, 3, width);
                close_in = mid1; close_cin = width; close_k = 3;
            }
            t.elems[out] = (int64_t)ho * wo * cout;
            const int wi_close = wi + n_own - 1;
            if (shortcut) weights(cout, 1, cin);
            if (shortcut && split) {
                t.elems[down] = t.elems[out];
                t.conv.push_back({cin, cout, 1, stride, hin, win, ho, wo, EPI_BIAS, x, -1, down, wi_short, -1, -1, 0, 0, 0, 0});
                t.conv.push_back({close_cin, cout, close_k, 1, ho, wo, ho, wo, EPI_RES_RELU, close_in, down, out, wi_close, -1, -1, 0, 0, 0, 0});
            } else if (shortcut) {
                t.conv.push_back({close_cin, cout, close_k, 1, ho, wo, ho, wo, EPI_RELU, close_in, -1, out, wi_close, x, wi_short, cin, stride, hin, win});
            } else {
                t.conv.push_back({close_cin, cout, close_k, 1, ho, wo, ho, wo, EPI_RES_RELU, close_in, x, out, wi_close, -1, -1, 0, 0, 0, 0});
            }
            wi += n_own + (shortcut ? 1 : 0);
            x = out; cin = cout; hin = ho; win = wo;
        }
    t.n_convs = wi;
    t.last_out = x;
    return t;
}

inline void rva_res_info(const rva_res_topo &t, size_t workspace_bytes, int32_t *maps, int64_t *ws, int32_t *n_launches)
{
    if (maps)
        for (int s = 0; s < 5; ++s) { maps[2 * s] = t.maps[s][0]; maps[2 * s + 1] = t.maps[s][1]; }
    if (ws) *ws = (int64_t)workspace_bytes;
    if (n_launches) *n_launches = 1 + (int32_t)t.conv.size() + 2;
}

// ResNet-18 (rva_resnet_plan_*, rva_resnet_f16_plan_*) as a case of it: BasicBlocks 2, 2, 2, 2 with the shortcut convolutions as
// launches of their own.  rva_resnet_weights::conv is already in the order of `convs` (per block conv1, conv2, shortcut).
inline rva_resnetx_desc rva_res18_desc(const rva_resnet_desc &d)
{
    return {d.height, d.width, d.classes, d.top_k, d.max_frames, 0, {2, 2, 2, 2}, RES_CONVS, RVA_RESX_SPLIT_SHORTCUT};
}

// the argument checks of a ResNet-18 create, under the entry's name; clears *out
inline int rva_res_check_args(rva_ctx *ctx, const char *who, const rva_resnet_desc *d, const rva_resnet_weights *wt, void **out)
{
    if (!ctx || !d || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (d->height < 1 || d->width < 1 || d->classes < 1 || d->classes > RVA_PLAN_MAX_CLASSES || d->top_k < 1 || d->max_frames < 1 ||
        d->max_frames > 65535 || (int64_t)d->height * d->width > (1 << 26))
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad descriptor (height, width >= 1, classes 1..%d, top_k >= 1, max_frames 1..65535)", who,
                        RVA_PLAN_MAX_CLASSES);
    bool all = wt->stem_w && wt->stem_b && wt->head_w && wt->head_b;
    for (int i = 0; i < RES_CONVS; ++i) all = all && wt->conv[i].w && wt->conv[i].b;
    if (!all) return rva_fail(ctx, RVA_ERR_ARG, "%s: every weight array is required", who);
    return RVA_OK;
}

// an RVA_RESNET_STAGE_* code as the stage code of that topology; -1: no such code
inline int rva_res18_stage(int stage)
{
    const auto slot = [](int b, int s) { return RVA_RESX_BLOCK0 + 4 * b + s; };
    if (stage == RVA_RESNET_STAGE_POOLED) return RVA_RESX_POOLED;
    if (stage == RVA_RESNET_STAGE_FEAT) return RVA_RESX_FEAT;
    if (stage >= RVA_RESNET_STAGE_MID0 && stage < RVA_RESNET_STAGE_DOWN2) return slot(stage - RVA_RESNET_STAGE_MID0, 0);
    if (stage >= RVA_RESNET_STAGE_DOWN2 && stage < RVA_RESNET_STAGE_OUT0) return slot(2 + 2 * (stage - RVA_RESNET_STAGE_DOWN2), 2);
    if (stage >= RVA_RESNET_STAGE_OUT0 && stage < RVA_RESNET_STAGE_FEAT) return slot(stage - RVA_RESNET_STAGE_OUT0, 3);
    return -1;
}

// ---------------------------------------------------------------------------------------------------
// 3D-CNN (rva_clip3d.hip, both precisions): conv1 + (1,2,2) pool, conv2 + (2,2,2) pool, conv3 + mean.  The pools floor.
constexpr int C3D_C1 = 64, C3D_C2 = 128, C3D_C3 = 256, C3D_TAPS = 27;
constexpr int C3D_PT = 8;                                  // pooled tile (PT x PT) of a K_conv1 block
constexpr int C3D_GROUPS = 32;                             // pool groups (of 8 conv positions) of a K_conv2 block; K_conv3: 256 positions
constexpr size_t C3D_W1 = (size_t)C3D_C1 * 3 * C3D_TAPS, C3D_W2 = (size_t)C3D_C2 * C3D_TAPS * C3D_C1, C3D_W3 = (size_t)C3D_C3 * C3D_TAPS * C3D_C2;

struct rva_c3d_geom {
    int T, H1, W1, T2, H2, W2;       // pool1 = (T, H1, W1), pool2 = (T2, H2, W2)
    int conv1_tiles_x, conv1_tiles, conv2_tiles, conv3_tiles;
    int64_t elems[4];                // elements of a RVA_CNN3D_STAGE_* per clip
};

inline rva_c3d_geom rva_c3d_geometry(const rva_cnn3d_desc &d)
{
    rva_c3d_geom g{};
    g.T = d.frames; g.H1 = d.height / 2; g.W1 = d.width / 2;
    g.T2 = g.T / 2; g.H2 = g.H1 / 2; g.W2 = g.W1 / 2;
    const int64_t ng = (int64_t)g.T2 * g.H2 * g.W2;
    g.conv1_tiles_x = rva_ceil_div(g.W1, C3D_PT);
    g.conv1_tiles = g.conv1_tiles_x * rva_ceil_div(g.H1, C3D_PT);
    g.conv2_tiles = (int)((ng + C3D_GROUPS - 1) / C3D_GROUPS);
    g.conv3_tiles = (int)((ng + 255) / 256);
    g.elems[RVA_CNN3D_STAGE_ACT1] = (int64_t)g.T * g.H1 * g.W1 * C3D_C1;
    g.elems[RVA_CNN3D_STAGE_ACT2] = ng * C3D_C2;
    g.elems[RVA_CNN3D_STAGE_PARTIAL] = (int64_t)g.conv3_tiles * C3D_C3;
    g.elems[RVA_CNN3D_STAGE_FEAT] = C3D_C3;
    return g;
}

// the argument checks of a create, under the entry's name; clears *out
inline int rva_c3d_check_args(rva_ctx *ctx, const char *who, const rva_cnn3d_desc *d, const rva_cnn3d_weights *wt, void **out)
{
    if (!ctx || !d || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    // the pools floor: (1,2,2) then (2,2,2) leave nothing of fewer than 2 frames or 4 rows / columns (torch fails there too)
    if (d->height < 4 || d->width < 4 || d->frames < 2 || d->classes < 1 || d->classes > RVA_PLAN_MAX_CLASSES || d->max_clips < 1 ||
        (int64_t)d->max_clips * d->frames > 65535 || (int64_t)d->height * d->width > (1 << 26))
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad descriptor (height, width >= 4, frames >= 2, classes 1..%d, max_clips >= 1, "
                        "max_clips * frames <= 65535)", who, RVA_PLAN_MAX_CLASSES);
    if (!wt->conv1_w || !wt->conv1_b || !wt->conv2_w || !wt->conv2_b || !wt->conv3_w || !wt->conv3_b || !wt->head_w || !wt->head_b)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: every weight array is required", who);
    return RVA_OK;
}

inline void rva_c3d_info(const rva_c3d_geom &g, int32_t *pool1, int32_t *pool2, int32_t *tiles, int32_t *n_launches)
{
    if (pool1) { pool1[0] = g.T; pool1[1] = g.H1; pool1[2] = g.W1; }
    if (pool2) { pool2[0] = g.T2; pool2[1] = g.H2; pool2[2] = g.W2; }
    if (tiles) { tiles[0] = g.conv1_tiles; tiles[1] = g.conv2_tiles; tiles[2] = g.conv3_tiles; }
    if (n_launches) *n_launches = 5;
}

// ---------------------------------------------------------------------------------------------------
// CNN-LSTM (rva_clip.hip, rva_clip_f16.hip; the host plan over both is rva_clip_host.h): per frame the stem (conv1 7x7 s2 p3 + pool
// 3x3 s2 p1) and conv2 3x3 p1 + mean, per clip a 2-layer LSTM and the head.
constexpr int CL_C1 = 64, CL_C2 = 128, CL_K1 = 7;          // stem widths of the architecture
constexpr int CL_PT = 8;                                   // pooled tile (PT x PT) of a K_stem block; K_conv2: 256 pixels
constexpr int CL_MAX_HIDDEN = 1024, CL_MAX_T = 64;
constexpr int CL_STAGES = RVA_CNNLSTM_STAGE_H2 + 1;

struct rva_cl_geom {
    int Hc, Wc, Hp, Wp;              // conv1's map and the pooled map
    int conv2_tiles;
    int64_t elems[CL_STAGES];        // elements of a RVA_CNNLSTM_STAGE_* per clip
    bool pitched[CL_STAGES];         // stored [T][max_clips][hidden]: fewer clips than the capacity are T rows out of that pitch
};

inline rva_cl_geom rva_cl_geometry(const rva_cnnlstm_desc &d)
{
    rva_cl_geom g{};
    rva_stem_maps(d.height, d.width, &g.Hc, &g.Wc, &g.Hp, &g.Wp);
    g.conv2_tiles = rva_ceil_div(g.Hp * g.Wp, 256);
    const int64_t T = d.frames;
    g.elems[RVA_CNNLSTM_STAGE_POOLED] = T * g.Hp * g.Wp * CL_C1;
    g.elems[RVA_CNNLSTM_STAGE_PARTIAL] = T * g.conv2_tiles * CL_C2;
    g.elems[RVA_CNNLSTM_STAGE_FEAT] = T * CL_C2;
    g.elems[RVA_CNNLSTM_STAGE_GX] = T * 4 * d.hidden;
    g.elems[RVA_CNNLSTM_STAGE_H1] = g.elems[RVA_CNNLSTM_STAGE_H2] = T * d.hidden;
    g.pitched[RVA_CNNLSTM_STAGE_H1] = g.pitched[RVA_CNNLSTM_STAGE_H2] = true;
    return g;
}

// The argument checks of a create, under the entry's name; clears *out.  `refuse_large`: the fp16 entry also refuses what its
// 16-bit grid rows and 32-bit frame offsets cannot hold.  The fp32 entry has never refused it, and a new refusal is a change of
// behaviour that wants its own change.
inline int rva_cl_check_args(rva_ctx *ctx, const char *who, bool refuse_large, const rva_cnnlstm_desc *d, const rva_cnnlstm_weights *wt,
                             void **out)
{
    if (!ctx || !d || !wt || !out) return rva_fail(ctx, RVA_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (d->height < 2 || d->width < 2 || d->frames < 1 || d->frames > CL_MAX_T || d->hidden < 1 || d->hidden > CL_MAX_HIDDEN ||
        d->classes < 1 || d->classes > RVA_PLAN_MAX_CLASSES || d->max_clips < 1 ||
        (refuse_large && ((int64_t)d->max_clips * d->frames > 65535 || (int64_t)d->height * d->width > (1 << 26))))
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad descriptor (frames 1..%d, hidden 1..%d, classes 1..%d, max_clips >= 1%s)", who, CL_MAX_T,
                        CL_MAX_HIDDEN, RVA_PLAN_MAX_CLASSES, refuse_large ? ", max_clips * frames <= 65535" : "");
    if (!wt->conv1_w || !wt->conv1_b || !wt->conv2_w || !wt->conv2_b || !wt->w_ih1 || !wt->b1 || !wt->w_hh1 || !wt->w_ih2 ||
        !wt->w_hh2 || !wt->b2 || !wt->head_w || !wt->head_b)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: every weight array is required", who);
    return RVA_OK;
}

// stem, conv2, mean, xproj; the frames + 1 diagonal LSTM launches; head
inline void rva_cl_info(const rva_cnnlstm_desc &d, const rva_cl_geom &g, int32_t *pooled_h, int32_t *pooled_w, int32_t *conv2_tiles,
                        int32_t *n_launches)
{
    if (pooled_h) *pooled_h = g.Hp;
    if (pooled_w) *pooled_w = g.Wp;
    if (conv2_tiles) *conv2_tiles = g.conv2_tiles;
    if (n_launches) *n_launches = 4 + (d.frames + 1) + 1;
}
