// The host side of the CNN-LSTM plan, written once for rva_clip.hip (fp32) and rva_clip_f16.hip (fp16): the plan object and its
// create / destroy / info / run / run_post / stage over the description of rva_plan_topo.h, each under the ABI entry's name.
//
// Each file defines its ABI handle P next to its kernels as `struct rva_..._plan : rva_cl_plan<E>`, E the element type of the
// frames, of `pooled` and of the convolution and LSTM weights, and adds what differs by precision:
//
//   REFUSE_LARGE                      rva_cl_check_args' flag; also whether create asks rva_plan_fits
//   pack(d, wt, w)                    rounds and packs the five weight arrays of E into `w` as the kernels read them; returns the
//                                     name of an array of which a value does not stay finite in E, or null
//   stem_prepare, stem, xproj, lstm   its stem's two launcher functions and its K_xproj / K_lstm kernels
//   conv2(n_frames, st)               launches its K_conv2
#pragma once

#include <type_traits>

#include "rva_lstm_dev.h"
#include "rva_plan_topo.h"

template <class E>
struct rva_cl_weights {
    std::vector<E> w1, w2, wih1, whh1, wl2;                // conv1, conv2, W_ih1, W_hh1, [W_ih2 | W_hh2]
};

template <class E>
struct rva_cl_plan {
    typedef E elem;
    rva_ctx *ctx = nullptr;
    rva_cnnlstm_desc d{};
    rva_cl_geom g{};
    E *w1 = nullptr, *w2 = nullptr, *wih1 = nullptr, *whh1 = nullptr, *wl2 = nullptr, *pooled = nullptr;
    float *b1 = nullptr, *b2 = nullptr, *bl1 = nullptr, *bl2 = nullptr, *wh = nullptr, *bh = nullptr;
    float *partial = nullptr, *feat = nullptr, *gx = nullptr, *h1 = nullptr, *h2 = nullptr, *c1 = nullptr, *c2 = nullptr;
    rva_dev_arena mem;
};

template <class P>
void rva_cl_destroy(P *p)
{
    if (!p) return;
    p->mem.release();
    delete p;
}

template <class P>
int rva_cl_create(rva_ctx *ctx, const char *who, const rva_cnnlstm_desc *desc, const rva_cnnlstm_weights *wt, P **out)
{
    typedef typename P::elem E;
    int rc = rva_cl_check_args(ctx, who, P::REFUSE_LARGE, desc, wt, (void **)out);
    if (rc != RVA_OK) return rc;
    const rva_cnnlstm_desc d = *desc;
    rva_cl_weights<E> w;
    if (const char *bad = P::pack(d, *wt, w)) return rva_fail(ctx, RVA_ERR_ARG, "%s: a value of %s does not stay finite in fp16", who, bad);
    const rva_cl_geom g = rva_cl_geometry(d);
    const int h = d.hidden, G4 = 4 * h, T = d.frames;
    const size_t mc = (size_t)d.max_clips;
    auto n = [&](int stage) { return mc * g.elems[stage]; };
    if (P::REFUSE_LARGE) {
        const size_t need = (n(RVA_CNNLSTM_STAGE_POOLED) + w.w1.size() + w.w2.size() + w.wih1.size() + w.whh1.size() + w.wl2.size()) * sizeof(E) +
                            (n(RVA_CNNLSTM_STAGE_PARTIAL) + n(RVA_CNNLSTM_STAGE_FEAT) + n(RVA_CNNLSTM_STAGE_GX) + n(RVA_CNNLSTM_STAGE_H1) +
                             n(RVA_CNNLSTM_STAGE_H2) + 2 * mc * h + CL_C1 + CL_C2 + 2 * (size_t)G4 + (size_t)d.classes * (h + 1)) * sizeof(float);
        char shape[64];
        snprintf(shape, sizeof shape, "%d clips of %d x %d x %d", d.max_clips, T, d.height, d.width);
        rc = rva_plan_fits(ctx, who, need, shape);
        if (rc != RVA_OK) return rc;
    }
    auto *p = new P();
    p->ctx = ctx;
    p->d = d;
    p->g = g;
    auto step = [&](int r) { if (rc == RVA_OK) rc = r; };
    step(p->mem.upload(ctx, &p->w1, w.w1.data(), w.w1.size()));
    step(p->mem.upload(ctx, &p->b1, wt->conv1_b, CL_C1));
    step(p->mem.upload(ctx, &p->w2, w.w2.data(), w.w2.size()));
    step(p->mem.upload(ctx, &p->b2, wt->conv2_b, CL_C2));
    step(p->mem.upload(ctx, &p->wih1, w.wih1.data(), w.wih1.size()));
    step(p->mem.upload(ctx, &p->bl1, wt->b1, G4));
    step(p->mem.upload(ctx, &p->whh1, w.whh1.data(), w.whh1.size()));
    step(p->mem.upload(ctx, &p->wl2, w.wl2.data(), w.wl2.size()));
    step(p->mem.upload(ctx, &p->bl2, wt->b2, G4));
    step(p->mem.upload(ctx, &p->wh, wt->head_w, (size_t)d.classes * h));
    step(p->mem.upload(ctx, &p->bh, wt->head_b, d.classes));
    step(p->mem.alloc(ctx, &p->pooled, n(RVA_CNNLSTM_STAGE_POOLED)));
    step(p->mem.alloc(ctx, &p->partial, n(RVA_CNNLSTM_STAGE_PARTIAL)));
    step(p->mem.alloc(ctx, &p->feat, n(RVA_CNNLSTM_STAGE_FEAT)));
    step(p->mem.alloc(ctx, &p->gx, n(RVA_CNNLSTM_STAGE_GX)));
    step(p->mem.alloc(ctx, &p->h1, n(RVA_CNNLSTM_STAGE_H1)));
    step(p->mem.alloc(ctx, &p->h2, n(RVA_CNNLSTM_STAGE_H2)));
    step(p->mem.alloc(ctx, &p->c1, mc * h));
    step(p->mem.alloc(ctx, &p->c2, mc * h));
    if (rc == RVA_OK) rc = P::stem_prepare(ctx);
    if (rc == RVA_OK && rva_func_smem((const void *)P::lstm, lstm_lds<E>(h)) != hipSuccess)
        rc = rva_fail(ctx, RVA_ERR_HIP, "%s: cannot raise the LSTM kernel's LDS limit", who);
    if (rc == RVA_OK) rc = rva_clip_head_prepare(ctx, h);
    if (rc == RVA_OK) rc = rva_clip_post_prepare(ctx, d.classes);
    if (rc != RVA_OK) {
        rva_cl_destroy(p);
        return rc;
    }
    *out = p;
    return RVA_OK;
}

template <class P>
int rva_cl_info(const P *p, int32_t *pooled_h, int32_t *pooled_w, int32_t *conv2_tiles, int32_t *n_launches)
{
    if (!p) return RVA_ERR_ARG;
    rva_cl_info(p->d, p->g, pooled_h, pooled_w, conv2_tiles, n_launches);
    return RVA_OK;
}

template <class P>
int rva_cl_run(P *p, const char *who, const void *frames, const int32_t *frame_index, int n_clips, void *logits, rva_stream_t stream_)
{
    typedef typename P::elem E;
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (!frames || !frame_index || !logits || n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad argument (n_clips %d, capacity %d)", who, n_clips, p->d.max_clips);
    const hipStream_t st = (hipStream_t)stream_;
    const rva_cl_geom &g = p->g;
    const int T = p->d.frames, h = p->d.hidden, G4 = 4 * h, nf = n_clips * T;
    int rc = P::stem(ctx, (const E *)frames, frame_index, p->w1, p->b1, p->pooled, p->d.height, p->d.width, nf, st);
    if (rc != RVA_OK) return rc;
    p->conv2(nf, st);
    RVA_HIP(ctx, hipGetLastError());
    rc = rva_clip_mean_launch(ctx, p->partial, g.conv2_tiles, (float)(g.Hp * g.Wp), p->feat, nf, CL_C2, st);
    if (rc != RVA_OK) return rc;
    P::xproj<<<dim3(rva_ceil_div(G4, 256), n_clips), 256, (size_t)T * CL_C2 * sizeof(float), st>>>(p->feat, p->wih1, p->bl1, p->gx, T, G4);
    RVA_HIP(ctx, hipGetLastError());
    for (int s = 0; s <= T; ++s) {
        P::lstm<<<dim3(rva_ceil_div(h, LSTM_U), 2), 256, lstm_lds<E>(h), st>>>(s, T, h, n_clips, p->d.max_clips, p->whh1, p->wl2, p->gx, p->bl2,
                                                                               p->h1, p->h2, p->c1, p->c2);
        RVA_HIP(ctx, hipGetLastError());
    }
    return rva_clip_head_launch(ctx, p->h2 + (size_t)(T - 1) * p->d.max_clips * h, p->wh, p->bh, (float *)logits, h, p->d.classes,
                                n_clips, st);
}

template <class P>
int rva_cl_run_post(P *p, const char *who, const void *logits, const int32_t *rows, int n_rows, int max_det, void *scores, void *cls,
                    void *boxes, void *counts, rva_stream_t stream_)
{
    if (!p) return RVA_ERR_ARG;
    return rva_clip_post_launch(p->ctx, who, (const float *)logits, p->d.classes, std::min(5, p->d.classes), rows, n_rows, max_det,
                                (float *)scores, (int32_t *)cls, (float *)boxes, (int32_t *)counts, (hipStream_t)stream_);
}

// Read-only tap on the workspace (tests and tools): one device-to-device copy, no kernel.  POOLED is elements of E, every other
// stage fp32, and the counts are element counts (the size error of an fp32 stage says "floats").  h1 / h2 keep max_clips rows per
// step, so fewer clips than the capacity are T rows of n_clips * hidden out of a pitch of max_clips * hidden: one 2D copy.
template <class P>
int rva_cl_stage(P *p, const char *who, int stage, int n_clips, void *dst, int64_t dst_elems, int64_t *n_elems, rva_stream_t stream_)
{
    typedef typename P::elem E;
    if (!p) return RVA_ERR_ARG;
    rva_ctx *ctx = p->ctx;
    if (n_clips < 1 || n_clips > p->d.max_clips)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad argument (n_clips %d, capacity %d)", who, n_clips, p->d.max_clips);
    if (stage < 0 || stage >= CL_STAGES) return rva_fail(ctx, RVA_ERR_ARG, "%s: unknown stage %d", who, stage);
    const void *const src[CL_STAGES] = {p->pooled, p->partial, p->feat, p->gx, p->h1, p->h2};
    const int64_t T = p->d.frames, h = p->d.hidden;
    const bool rows = p->g.pitched[stage] && n_clips < p->d.max_clips;
    const bool as_e = stage == RVA_CNNLSTM_STAGE_POOLED && !std::is_same<E, float>::value;
    return rva_clip_stage_copy(ctx, who, stage, n_clips, "clips", src[stage], as_e ? sizeof(E) : sizeof(float), as_e ? "elements" : "floats",
                               n_clips * p->g.elems[stage], rows ? T : 0, n_clips * h, p->d.max_clips * h, dst, dst_elems, n_elems,
                               (hipStream_t)stream_);
}
