// rva_yolov8_plan_*: the fused YOLOv8 detector as ONE object behind the C ABI.
//
// Replaces the reference's `session.run` (detector.py:597-609: ONNX Runtime on the exported ultralytics graph) in fp16 or, with
// RVA_PLAN_F32, in the reference's own fp32 (the same graph on fp32 buffers and the kernels of rva_conv_f32.hip, see build()):
// create() takes the network's convolutions in module order (BatchNorm folded, the checkpoint's own fp32 [Cout][Cin][k][k]
// layout), packs them for the kernels of rva_conv.hip, allocates every NHWC fp16 activation buffer in HBM and lays down the static
// list of launches (one per Conv-BN-SiLU; concat / chunk / upsample never materialise: producers write channel slices of the
// concat buffers, consumers read slices through a row stride); run() replays that list -- one ABI call per forward pass.  The
// per-layer kernel variant is a field of each step: a tuner (engine.py) times the applicable variants through
// rva_yolov8_plan_launch_tunable and fixes its choice with rva_yolov8_plan_set_variant; without a tuner every step uses the
// library's heuristic (variant 0).  No host synchronisation, no allocation after create(): a run can be captured into a hipGraph.
//
// Static rows (rva_yolov8_plan_set_static_rows): a letterboxed frame leaves the same border rows in `input` on every run, and the
// output rows of the early layers whose receptive field lies in the border (and the zero padding) come out the same every time.
// Every step carries the window [y0, y1) of its output rows that can change, propagated from the input window through the step
// list (propagate_rows); after one complete run over all rows has filled every buffer ("primed"), the steps whose kernel takes a
// row window launch that window only.  The rows outside it keep the bytes of the priming run.
//
// Capacity (rva_yolov8_plan_run_n): desc.batch is the number of images the buffers hold, and a run takes the n <= batch leading
// ones.  Image b lies where it lies in a full run (NHWC: an image's offset does not depend on the batch), every step launches
// the kernel a full run launches (a fixed variant is one kernel; variant 0 chooses from the capacity, rva_conv2d_nhwc_f16_sel;
// the fp32 kernels give the same bits for every tile and batch), so images [0, n) come out bit for bit as in a full run and
// nothing of the images behind them is written.  "Primed" is therefore a count: the leading images whose buffers hold a whole
// run's rows.
//
// Graph (ultralytics YOLOv8 n / s / m / l / x: widths c1..c5, C2f depths, nc classes, reg_max 16):
//   b0 stem 3x3 s2 | b1 3x3 s2 | b2 C2f | b3 3x3 s2 | b4 C2f | b5 3x3 s2 | b6 C2f | b7 3x3 s2 | b8 C2f | b9 SPPF |
//   h12 C2f(cat[up(p5), p4]) | h15 C2f(cat[up(n4), p3]) | h16 3x3 s2 | h18 C2f(cat[h16, n4]) | h19 3x3 s2 | h21 C2f(cat[h19, p5]) |
//   detect: per level box = 3x3, 3x3, 1x1 (4 reg_max) and cls = 3x3, 3x3, 1x1 (nc); DFL + dist2bbox + sigmoid -> [B, 4+nc, A].
// Class count: any 1 <= nc <= 1024.  The class branch runs with its channel counts rounded up to what the kernels take (interior
// width to 8, to 16 in an fp32 plan; the logits to ncp = roundup(nc, 8) columns), weights and biases zero-extended on the host
// before they are packed (Builder::padded): a pad channel is SiLU(0) = 0 and meets zero weights.  The head kernels read rows of
// ncp logits and store the nc real class rows, so the output is exactly [B, 4+nc, A].
// Module order of `convs` (what create() consumes, checked against the descriptor): b0, b1, C2f(b2), b3, C2f(b4), b5, C2f(b6), b7,
// C2f(b8), SPPF(b9) = cv1, cv2, C2f(h12), C2f(h15), h16, C2f(h18), h19, C2f(h21), then per level l = 0..2: box[l][0..2], then per
// level: cls[l][0..2];  C2f(x) = cv1, cv2, then per bottleneck: cv1, cv2.
//
// rva_yolov5_plan_create and rva_yolo11_plan_create lay down the graphs of YOLOv5 and YOLO11 for the same plan object (the graphs
// and module orders are in include/rva.h).  YOLO11 adds two step kinds, K_DWCONV and K_ATTN (rva_attn.hip): fixed kernels like the
// pooling steps, and in propagate_rows always the whole map -- attention is global.
//
// How a graph is laid down.  The three entry points check what is their architecture's, fill the internal descriptor and hand
// create_plan() the graph to build; everything else of a create (common checks, ownership, error codes, events, the starting
// state) is there once.  Builder::build / build_v5 / build_11 are compositions of the same parts, each a member of Builder that
// takes the family's block as a callable `block(i, src, dst, level, name)`:
//   stem (3x3 or 6x6; fp16 two launches, fp16 fused with b1, fp32) | backbone (block, 3 x [3x3 s2, block], SPPF; sets quiet_step) |
//   top_down (the fold-the-upsampling decision, else upsampling steps; YOLOv8, YOLO11) | bottom_up (2 x [3x3 s2, block]; notes the
//   fork points) | head_open / head_last / head_close (YOLOv8, YOLO11: widths, box branches, last 1x1 with or without the decode).
// The blocks: c2f (the C2f skeleton: YOLOv8's C2f with `pair` inside, YOLO11's C3k2 with `bottleneck` at half width or `c3` inside),
// c3 (YOLOv5's C3, YOLO11's C3k), sppf, c2psa.  A block's input is a Src: a view, or (low, skip) for cat[up(low), skip]; conv_in
// emits the one or the other.  Geo holds the batch, the widths and the five pyramid levels: buffers and steps name a level.
#include <algorithm>
#include <cstring>
#include <deque>
#include <memory>

#include "rva_internal.h"

namespace {

enum StepKind { K_CONV, K_UPCAT, K_HEAD, K_STEM2, K_STEM, K_SPPF3, K_POOL5, K_UP2, K_HEAD3, K_PAIR32,
                K_CONV_F32, K_STEM_F32, K_POOL5_F32, K_UP2_F32, K_HEAD_F32, K_STEM6, K_HEAD5, K_DWCONV, K_ATTN };

struct View {           // a channel slice of an NHWC buffer (es = bytes per element: 2 fp16, 4 fp32)
    char *base = nullptr; int ld = 0, off = 0, ch = 0, es = 2;
    void *ptr() const { return base + (size_t)es * off; }
    View sub(int o, int c) const { View v = *this; v.off += o; v.ch = c; return v; }
};

struct Step {
    StepKind kind;
    int lane = 0;                         // 0 = main stream, 1 / 2 = side stream of a detect branch
    int tunable = -1;                     // index into plan->tunables, -1 = fixed kernel
    const void *in = nullptr, *in2 = nullptr; int ldi = 0, ldi2 = 0, c_in = 0, c_in2 = 0;
    const void *w = nullptr, *w2 = nullptr; const float *b = nullptr, *b2 = nullptr;
    void *out = nullptr, *out2 = nullptr, *out3 = nullptr; int ldo = 0;
    const void *res = nullptr; int ldr = 0;
    int H = 0, W = 0, Cin = 0, Cout = 0, k = 0, stride = 0, act = 0, variant = 0;
    int mode = 0, a0 = 0; float stride_px = 0.f;
    int c_real = 0;                       // K_CONV: input channels before padding (what the step really depends on)
    int Ho = 0, y0 = 0, y1 = 0;           // output rows, and the window of them that depends on the non-static input rows
    // head3
    const void *hb[3] = {nullptr, nullptr, nullptr}, *hk[3] = {nullptr, nullptr, nullptr};
    int32_t hldb[3] = {0, 0, 0}, hldc[3] = {0, 0, 0}, hh[3] = {0, 0, 0}, hw[3] = {0, 0, 0}; float hs[3] = {0, 0, 0};
};

struct Tunable { int step; std::string base, desc; };      // desc = base (+ the step's row window where it is not the whole image)

}  // namespace

struct rva_yolov8_plan {
    rva_ctx *ctx = nullptr;
    rva_yolov8_desc d{};
    int B = 0, H = 0, W = 0, nc = 0, A = 0;
    int head_rows = 0;                    // rows of the head tensor: 4 + nc (YOLOv8), 5 + nc (YOLOv5)
    std::vector<void *> allocs;
    std::vector<Step> steps;
    std::vector<Tunable> tunables;
    int fork_step[3] = {-1, -1, -1};      // lane l forks off the main stream in front of this step
    int quiet_step = 0;
    hipEvent_t fork_ev[3] = {nullptr, nullptr, nullptr}, join_ev[3] = {nullptr, nullptr, nullptr};
    bool fused_stem = false, fused_head = false;
    bool f32 = false;                     // RVA_PLAN_F32: fp32 buffers and the kernels of rva_conv_f32.hip
    bool box32 = false;                   // RVA_PLAN_BOX_F32: the head kernels also write the box rows as fp32 [B, 4, A] behind the fp16 head
    size_t box_off = 0;                   // ... at this byte offset of `output` (rva_yolov8_plan_output_layout)
    int rows_top = 0, rows_bottom = 0;    // input rows outside [top, bottom) are static (set_static_rows); (0, H) = none
    bool windowed = false;                // some step's window is smaller than its image
    int primed = 0;                       // leading images whose buffers hold a whole run's rows for the current windows and variants
};

namespace {

struct Geo {            // computed once per plan: the batch, the widths c[1..5] and the pyramid levels l = 1..5 (the input at stride 2^l)
    int B = 0, H = 0, W = 0, c[6] = {}, h[6] = {}, w[6] = {};
    explicit Geo(const rva_yolov8_desc &d) : B(d.batch), H(d.height), W(d.width)
    {
        for (int l = 1; l <= 5; ++l) { c[l] = d.widths[l - 1]; h[l] = H >> l; w[l] = W >> l; }
    }
    float stride(int l) const { return (float)(1 << l); }
    int a0(int l) const { return l <= 3 ? 0 : a0(l - 1) + h[l - 1] * w[l - 1]; }      // grid cells of the detect levels 3 .. l - 1
};

struct Src {            // what a block reads: one view, or (low, skip) standing for cat([upsample2x(low), skip])
    View v, low; bool up = false;
    Src(View x) : v(x) {}
    Src(View l, View skip) : v(skip), low(l), up(true) {}
    int ch() const { return up ? low.ch + v.ch : v.ch; }
};

struct Head {           // the detect head of YOLOv8 and YOLO11: widths, the box branches' convolutions, the decode step over all levels
    int rm4, cb, cc_real, cc, ncp;        // 4 reg_max | box branch | class branch as the checkpoint has it, as it runs | logit columns
    const rva_conv_weights *box[3][3];
    Step h3s;
};

struct Builder {
    rva_yolov8_plan *p;
    const rva_conv_weights *convs;
    const Geo g;
    int next = 0;                         // next convolution of the module-order list
    int lane = 0;
    int fork_at[2] = {-1, -1};            // the steps in front of which n3 / m4 are complete (bottom_up)
    std::string err;                      // the first failure; nothing is launched and every builder returns false once it is set
    bool hip_failed = false;              // ... and whether it was a HIP call that failed
    std::deque<std::vector<float>> pad_store;             // zero-extended host copies of the class branch (padded) ...
    std::deque<rva_conv_weights> pad_convs;               // ... and their descriptors

    Builder(rva_yolov8_plan *plan, const rva_conv_weights *cv) : p(plan), convs(cv), g(plan->d) {}

    bool fail(const std::string &m, bool hip = false)
    {
        if (err.empty()) { err = m; hip_failed = hip; }
        return false;
    }

    void *dev_alloc(size_t bytes, bool zero)
    {
        void *ptr = nullptr;
        if (hipMalloc(&ptr, bytes ? bytes : 16) != hipSuccess) { fail("hipMalloc failed", true); return nullptr; }
        p->allocs.push_back(ptr);
        if (zero && hipMemset(ptr, 0, bytes) != hipSuccess) { fail("hipMemset failed", true); return nullptr; }
        return ptr;
    }
    // a zeroed activation buffer of level l, ch channels wide (a failed allocation is in `err`: the next pack() stops the builder)
    View buf(int l, int ch)
    {
        View v;
        // + 64 B: a convolution whose Cin is not a multiple of 32 runs with Cin rounded up (zero weights for the extra channels, see
        // conv()) and reads up to 31 channels past its slice -- the next slice of the row, the next row, or, behind the last row, this slack
        v.es = p->f32 ? 4 : 2;
        v.base = (char *)dev_alloc((size_t)g.B * g.h[l] * g.w[l] * ch * v.es + 64, true);
        v.ld = ch; v.off = 0; v.ch = ch;
        return v;
    }
    bool upload(const void *host, size_t bytes, const void **dev, const char *what = "weight")
    {
        void *d = dev_alloc(bytes, false);
        if (!d) return false;
        if (hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(std::string(what) + " upload failed", true);
        *dev = d;
        return true;
    }
    // a weight / bias pair
    bool upload(const void *w, size_t w_bytes, const std::vector<float> &b, const void **dw, const float **db, const char *what = "weight")
    {
        const void *d = nullptr;
        if (!upload(w, w_bytes, dw, what) || !upload(b.data(), b.size() * sizeof(float), &d, what)) return false;
        *db = (const float *)d;
        return true;
    }
    // Pack sibling convolutions (equal Cin / kernel / stride, outputs concatenated) as [CoutPad][k*k][CinPad] T + [CoutPad] fp32 into
    // (s.w, s.b) with the shape, or with `second` into (s.w2, s.b2) alone.  pad: Cout up to rva_conv_cout_pad, Cin up to 32
    template <typename T>
    bool pack_as(const rva_conv_weights *const *cv, int n, bool pad, Step &s, bool second)
    {
        if (!err.empty()) return false;   // a take() or a buffer in front of this step failed
        const rva_conv_weights &c0 = *cv[0];
        int co = 0;
        for (int i = 0; i < n; ++i) {
            if (!cv[i]->weight || cv[i]->cin != c0.cin || cv[i]->k != c0.k || cv[i]->stride != c0.stride) return fail("sibling convolutions differ");
            co += cv[i]->cout;
        }
        const int kk = c0.k * c0.k, cpad = pad ? rva_conv_cout_pad(co) : co, cinp = pad ? (c0.cin + 31) / 32 * 32 : c0.cin;
        std::vector<T> hw((size_t)cpad * kk * cinp, (T)0.f);
        std::vector<float> hb(cpad, 0.f);
        int o = 0;
        for (int i = 0; i < n; ++i) {
            const rva_conv_weights &c = *cv[i];
            for (int oc = 0; oc < c.cout; ++oc) {
                for (int ic = 0; ic < c.cin; ++ic)
                    for (int t = 0; t < kk; ++t)
                        hw[((size_t)(o + oc) * kk + t) * cinp + ic] = (T)c.weight[((size_t)oc * c.cin + ic) * kk + t];
                if (c.bias) hb[o + oc] = c.bias[oc];
            }
            o += c.cout;
        }
        if (!upload(hw.data(), hw.size() * sizeof(T), hb, second ? &s.w2 : &s.w, second ? &s.b2 : &s.b)) return false;
        if (!second) { s.Cin = c0.cin; s.Cout = co; s.k = c0.k; s.stride = c0.stride; }
        return true;
    }
    // fp16 padded for the kernels of rva_conv.hip; an fp32 plan as it is (rva_conv2d_nhwc_f32_v masks the tile edges)
    bool pack(const rva_conv_weights *const *cv, int n, Step &s, bool second = false)
    {
        return p->f32 ? pack_as<float>(cv, n, false, s, second) : pack_as<_Float16>(cv, n, true, s, second);
    }
    const rva_conv_weights *take(int cin, int cout, int k, int stride, const char *what)
    {
        if (next >= p->d.n_convs) { fail(std::string("convolution list too short at ") + what); return nullptr; }
        const rva_conv_weights *c = &convs[next++];
        if (c->cin != cin || c->cout != cout || c->k != k || c->stride != stride) {
            char m[200];
            snprintf(m, sizeof m, "convolution %d (%s): expected %d->%d k%d s%d, got %d->%d k%d s%d", next - 1, what, cin, cout, k, stride,
                     c->cin, c->cout, c->k, c->stride);
            fail(m);
            return nullptr;
        }
        return c;
    }
    bool all_taken() { return next == p->d.n_convs || fail("convolution list longer than the architecture"); }
    // `c` with input / output channels zero-extended to cinp / coutp (the convolution itself where nothing is to pad)
    const rva_conv_weights *padded(const rva_conv_weights *c, int cinp, int coutp)
    {
        if (!c || !c->weight || (c->cin == cinp && c->cout == coutp)) return c;
        const int kk = c->k * c->k;
        std::vector<float> &w = pad_store.emplace_back((size_t)coutp * cinp * kk, 0.f);
        for (int oc = 0; oc < c->cout; ++oc)
            for (int ic = 0; ic < c->cin; ++ic)
                memcpy(&w[((size_t)oc * cinp + ic) * kk], &c->weight[((size_t)oc * c->cin + ic) * kk], sizeof(float) * kk);
        rva_conv_weights q = *c;
        q.weight = w.data(); q.cin = cinp; q.cout = coutp;
        if (c->bias) {
            std::vector<float> &b = pad_store.emplace_back((size_t)coutp, 0.f);
            memcpy(b.data(), c->bias, sizeof(float) * c->cout);
            q.bias = b.data();
        }
        return &pad_convs.emplace_back(q);
    }
    void push(Step &s, const char *desc_fmt, ...)
    {
        s.lane = lane;
        if (desc_fmt) {
            char d[96];
            va_list ap; va_start(ap, desc_fmt); vsnprintf(d, sizeof d, desc_fmt, ap); va_end(ap);
            s.tunable = (int)p->tunables.size();
            p->tunables.push_back(Tunable{(int)p->steps.size(), d, d});
        }
        p->steps.push_back(s);
    }

    // ---------------------------------------------------------------------------------------------- steps
    // one Conv-BN-SiLU (or a fused group of siblings) on a level-l input; returns false on error
    bool conv(const rva_conv_weights *const *cv, int n, View src, View dst, int l, int act, const View *res = nullptr)
    {
        Step s{}; s.kind = p->f32 ? K_CONV_F32 : K_CONV;
        if (!pack(cv, n, s)) return false;
        if (s.Cin != src.ch || s.Cout != dst.ch) return fail("convolution does not fit its buffers");
        s.in = src.ptr(); s.ldi = src.ld; s.out = dst.ptr(); s.ldo = dst.ld; s.H = g.h[l]; s.W = g.w[l]; s.act = act;
        if (res) { s.res = res->ptr(); s.ldr = res->ld; }
        s.c_real = s.Cin;
        if (p->f32) {                     // every channel count is read as it is: the kernel never reads past its slice
            if (s.Cin % 16) return fail("fp32 plan: convolution input channels must be multiples of 16");
        } else if (s.Cin % 32 && !(p->d.flags & RVA_PLAN_NO_CIN_PAD)) {
            // Cin 48 / 16 (YOLOv8m / n): the LDS-DMA kernels want whole 32-channel chunks.  The packed weights already carry zero
            // columns up to the next multiple of 32, so the step simply declares the padded Cin: the extra channels it reads are whatever
            // follows the slice (finite activations of the neighbouring slice / pixel, or the buffer's zero slack) times zero.
            s.Cin = (s.Cin + 31) / 32 * 32;
        }
        push(s, "%d->%d k%ds%d %dx%d", s.c_real, s.Cout, s.k, s.stride, s.H, s.W);
        return true;
    }
    bool conv1(const rva_conv_weights *c, View src, View dst, int l, int act, const View *res = nullptr)
    {
        return c && conv(&c, 1, src, dst, l, act, res);
    }
    // the 1x1 convolution(s) a block opens with: plain, or with the upsample + concat folded in (rva_conv1x1_upcat_f16)
    bool conv_in(const rva_conv_weights *const *cv, int n, const Src &src, View dst, int l)
    {
        if (!src.up) return conv(cv, n, src.v, dst, l, 1);
        const View &low = src.low, &skip = src.v;
        Step s{}; s.kind = K_UPCAT;
        if (!pack(cv, n, s)) return false;
        if (s.k != 1 || s.stride != 1 || s.Cin != src.ch() || s.Cout != dst.ch) return fail("upsample + concat convolution does not fit");
        s.in = low.ptr(); s.ldi = low.ld; s.c_in = low.ch; s.in2 = skip.ptr(); s.ldi2 = skip.ld; s.c_in2 = skip.ch;
        s.out = dst.ptr(); s.ldo = dst.ld; s.H = g.h[l]; s.W = g.w[l]; s.act = 1;
        push(s, "up%d+%d->%d k1s1 %dx%d", low.ch, skip.ch, s.Cout, s.H, s.W);
        return true;
    }
    // 1x1 convolution + decode of a detect branch (mode 1: box, 2: class) at level l, into the level's anchor range of the output
    bool head(const rva_conv_weights *c, View src, int mode, int l)
    {
        if (!c) return false;
        Step s{}; s.kind = K_HEAD;
        if (!pack(&c, 1, s)) return false;
        if (s.k != 1 || s.stride != 1 || s.Cin != src.ch) return fail("head convolution does not fit");
        s.in = src.ptr(); s.ldi = src.ld; s.H = g.h[l]; s.W = g.w[l]; s.mode = mode; s.a0 = g.a0(l); s.stride_px = g.stride(l);
        push(s, "head%d:%d->%d k1s1 %dx%d", mode, s.Cin, s.Cout, s.H, s.W);
        return true;
    }
    // nearest 2x upsampling of the level-l map src into dst (level l - 1)
    void up2(View src, View dst, int l)
    {
        Step s{}; s.kind = p->f32 ? K_UP2_F32 : K_UP2; s.in = src.ptr(); s.ldi = src.ld; s.out = dst.ptr(); s.ldo = dst.ld;
        s.H = g.h[l]; s.W = g.w[l]; s.Cin = src.ch;
        push(s, nullptr);
    }
    // Depthwise 3x3 (rva_dwconv3x3_nhwc_f16) over channels [c_off, c_off + dst.ch) of `c` (weight [C][1][3][3]): weights repacked
    // [9][dst.ch] fp16 (tap major).  Untunable; always the whole map.
    bool dwconv(const rva_conv_weights *c, int c_off, View src, View dst, int l, int act, const View *res = nullptr)
    {
        const int C = dst.ch;
        if (!c) return false;
        if (!c->weight || c->cin != 1 || c->k != 3 || c->stride != 1 || c_off < 0 || c_off + C > c->cout || src.ch != C || C % 8)
            return fail("depthwise convolution does not fit its buffers");
        std::vector<_Float16> hw((size_t)9 * C);
        std::vector<float> hb(C, 0.f);
        for (int ch = 0; ch < C; ++ch) {
            for (int t = 0; t < 9; ++t) hw[(size_t)t * C + ch] = (_Float16)c->weight[(size_t)(c_off + ch) * 9 + t];
            if (c->bias) hb[ch] = c->bias[c_off + ch];
        }
        Step s{}; s.kind = K_DWCONV;
        if (!upload(hw.data(), hw.size() * 2, hb, &s.w, &s.b)) return false;
        s.in = src.ptr(); s.ldi = src.ld; s.out = dst.ptr(); s.ldo = dst.ld; s.H = g.h[l]; s.W = g.w[l]; s.Cin = s.Cout = C; s.k = 3; s.stride = 1; s.act = act;
        if (res) { s.res = res->ptr(); s.ldr = res->ld; }
        push(s, nullptr);
        return true;
    }

    // ---------------------------------------------------------------------------------------------- blocks
    // Bottleneck y = cv2_3x3(cv1_k1xk1(x)) (+ x) through cmid channels.  The intermediate is a buffer of this bottleneck alone: with
    // row windows a step rewrites part of its output only, and the rest must still be what THIS bottleneck's first convolution left
    // there (the second one reads it as halo)
    bool bottleneck(View x, View y, int cmid, bool shortcut, int l, const char *what, int k1 = 3)
    {
        const rva_conv_weights *b1 = take(x.ch, cmid, k1, 1, what), *b2 = take(cmid, y.ch, 3, 1, what);
        View tmp = buf(l, cmid);
        return conv1(b1, x, tmp, l, 1) && conv1(b2, tmp, y, l, 1, shortcut ? &x : nullptr);
    }
    // C2f's bottleneck, 3x3 and 3x3 at full width; 32 channels wide with a shortcut both convolutions and the shortcut are one
    // launch, the intermediate in LDS (rva_c2f_pair32_f16)
    bool pair(View x, View y, bool shortcut, int l, const char *what)
    {
        const int c = x.ch;
        if (c != 32 || !shortcut || p->f32 || (p->d.flags & RVA_PLAN_NO_PAIR32)) return bottleneck(x, y, c, shortcut, l, what);
        const rva_conv_weights *b1 = take(c, c, 3, 1, what), *b2 = take(c, c, 3, 1, what);
        Step s{}; s.kind = K_PAIR32;
        if (!b1 || !b2 || !pack(&b1, 1, s) || !pack(&b2, 1, s, true)) return false;
        s.in = x.ptr(); s.ldi = x.ld; s.out = y.ptr(); s.ldo = y.ld; s.H = g.h[l]; s.W = g.w[l]; s.act = 1;
        push(s, nullptr);
        return true;
    }
    // The C2f skeleton (YOLOv8's C2f, YOLO11's C3k2): cv1 into the front 2c channels of one concat buffer, n inner blocks
    // inner(x = cat[(1 + i) c, c), y = cat[(2 + i) c, c)), cv2 over the whole buffer
    template <typename Inner>
    bool c2f(int c, int n, const Src &src, View dst, int l, const char *what, Inner inner)
    {
        const rva_conv_weights *cv1 = take(src.ch(), 2 * c, 1, 1, what), *cv2 = take((2 + n) * c, dst.ch, 1, 1, what);
        if (!cv1 || !cv2) return false;
        View cat = buf(l, (2 + n) * c);
        if (!conv_in(&cv1, 1, src, cat.sub(0, 2 * c), l)) return false;
        for (int i = 0; i < n; ++i)
            if (!inner(cat.sub((1 + i) * c, c), cat.sub((2 + i) * c, c))) return false;
        return conv1(cv2, cat, dst, l, 1);
    }
    // YOLOv5's C3 and, with k1 = 3, YOLO11's C3k (k1: kernel of every bottleneck's first convolution).  cv1 and cv2 read the same
    // input: one sibling launch writes cat[0, 2c) = [cv1 out | cv2 out]; the bottlenecks x <- x + cv2_3x3(cv1(x)) start from cv1 out,
    // every one but the last writes a buffer of its own (one writer per slice, see bottleneck), the last one cat[2c, 3c), and cv3
    // reads cat[c, 3c) = [cv2 out | m out] with the halves of its input channels swapped on the host (the module concatenates
    // [m out | cv2 out]).
    bool c3(int n, bool shortcut, const Src &src, View dst, int l, const char *what, int k1 = 1)
    {
        const int c2 = dst.ch, c = c2 / 2;
        const rva_conv_weights *cv[2] = {take(src.ch(), c, 1, 1, what), take(src.ch(), c, 1, 1, what)};
        const rva_conv_weights *cv3 = take(2 * c, c2, 1, 1, what);
        if (!cv[0] || !cv[1] || !cv3 || n < 1) return n < 1 ? fail("a C3 block needs at least one bottleneck") : false;
        View cat = buf(l, 3 * c);
        if (!conv_in(cv, 2, src, cat.sub(0, 2 * c), l)) return false;
        View x = cat.sub(0, c);
        for (int i = 0; i < n; ++i) {
            View y = i == n - 1 ? cat.sub(2 * c, c) : buf(l, c);
            if (!bottleneck(x, y, c, shortcut, l, what, k1)) return false;
            x = y;
        }
        if (!cv3->weight) return fail("convolution without weights");
        std::vector<float> &sw = pad_store.emplace_back((size_t)c2 * 2 * c, 0.f);
        for (int oc = 0; oc < c2; ++oc)
            for (int ic = 0; ic < 2 * c; ++ic) sw[(size_t)oc * 2 * c + ic] = cv3->weight[(size_t)oc * 2 * c + (ic + c) % (2 * c)];
        rva_conv_weights q = *cv3;
        q.weight = sw.data();
        return conv1(&pad_convs.emplace_back(q), cat.sub(c, 2 * c), dst, l, 1);
    }
    // SPPF at level 5: cv1, three chained 5x5 max pools into the slices of one concat buffer, cv2
    bool sppf(View src, View dst)
    {
        const int c5 = src.ch, c_ = c5 / 2, h5 = g.h[5], w5 = g.w[5];
        const rva_conv_weights *cv1 = take(c5, c_, 1, 1, "b9.cv1"), *cv2 = take(4 * c_, c5, 1, 1, "b9.cv2");
        View cat = buf(5, 4 * c_);
        if (!conv1(cv1, src, cat.sub(0, c_), 5, 1)) return false;
        if (h5 * w5 <= 2400 && !p->f32) {
            Step s{}; s.kind = K_SPPF3; s.in = cat.sub(0, c_).ptr(); s.ldi = cat.ld; s.out = cat.sub(c_, c_).ptr(); s.out2 = cat.sub(2 * c_, c_).ptr();
            s.out3 = cat.sub(3 * c_, c_).ptr(); s.ldo = cat.ld; s.H = h5; s.W = w5; s.Cin = c_;
            push(s, nullptr);
        } else {
            for (int i = 0; i < 3; ++i) {
                Step s{}; s.kind = p->f32 ? K_POOL5_F32 : K_POOL5; s.in = cat.sub(i * c_, c_).ptr(); s.ldi = cat.ld; s.out = cat.sub((i + 1) * c_, c_).ptr(); s.ldo = cat.ld;
                s.H = h5; s.W = w5; s.Cin = c_;
                push(s, nullptr);
            }
        }
        return conv1(cv2, cat, dst, 5, 1);
    }
    // YOLO11's C2PSA at level 5.  Every buffer slice has ONE writer (a windowed convolution rewrites part of its output only, see
    // bottleneck), so cv1 runs as two launches: `a` goes straight into cv2's input buffer, `b` into a buffer of its own, and the last
    // block's ffn writes the other half of cv2's input.  Attention and the positional encoding always run the whole map.
    bool c2psa(int n, int heads, View src, View dst)
    {
        const int c1 = src.ch, c = c1 / 2, l = 5;
        if (n < 1 || heads * 64 != c) return fail("C2PSA: psa_heads * 64 must be half the width of the block, and psa_blocks >= 1");
        const rva_conv_weights *cv1 = take(c1, 2 * c, 1, 1, "10.cv1"), *cv2 = take(2 * c, c1, 1, 1, "10.cv2");
        if (!cv1 || !cv2) return false;
        if (!cv1->weight) return fail("convolution without weights");
        rva_conv_weights qa = *cv1, qb = *cv1;
        qa.cout = qb.cout = c;
        qb.weight = cv1->weight + (size_t)c * c1;
        if (cv1->bias) qb.bias = cv1->bias + c;
        View cat = buf(l, 2 * c), x = buf(l, c);
        if (!conv1(&pad_convs.emplace_back(qa), src, cat.sub(0, c), l, 1) || !conv1(&pad_convs.emplace_back(qb), src, x, l, 1)) return false;
        for (int i = 0; i < n; ++i) {
            const rva_conv_weights *qkv = take(c, 2 * c, 1, 1, "10.attn.qkv"), *proj = take(c, c, 1, 1, "10.attn.proj"), *pe = take(1, c, 3, 1, "10.attn.pe"),
                                   *f0 = take(c, 2 * c, 1, 1, "10.ffn.0"), *f1 = take(2 * c, c, 1, 1, "10.ffn.1");
            if (!qkv || !proj || !pe || !f0 || !f1) return false;
            View q = buf(l, 2 * c), ao = buf(l, c), xo = buf(l, c), x1 = buf(l, c), f = buf(l, 2 * c);
            View y = i == n - 1 ? cat.sub(c, c) : buf(l, c);
            if (!conv1(qkv, x, q, l, 0)) return false;
            Step s{}; s.kind = K_ATTN; s.in = q.ptr(); s.ldi = q.ld; s.out = ao.ptr(); s.ldo = ao.ld; s.H = g.h[l]; s.W = g.w[l]; s.Cin = 2 * c; s.Cout = c; s.mode = heads;
            push(s, nullptr);
            for (int hd = 0; hd < heads; ++hd) {            // a head's v slice is contiguous, the heads' are not: one launch per head
                const View r = ao.sub(64 * hd, 64);
                if (!dwconv(pe, 64 * hd, q.sub(128 * hd + 64, 64), xo.sub(64 * hd, 64), l, 0, &r)) return false;
            }
            if (!conv1(proj, xo, x1, l, 0, &x)) return false;
            if (!conv1(f0, x1, f, l, 1) || !conv1(f1, f, y, l, 0, &x1)) return false;
            x = y;
        }
        return conv1(cv2, cat, dst, l, 1);
    }

    // ---------------------------------------------------------------------------------------------- graph parts
    // In every part `block(i, src, dst, l, what)` lays down the family's block i = 0 .. 7 (four of the backbone, two top-down, two
    // bottom-up) from src into dst at level l, and `what` names the convolutions in the family's module numbering.
    //
    // x1 = b1(b0(input)): the stem from the planar input K1 writes (k0 x k0, stride 2) and the 3x3 s2 behind it.
    bool stem(int k0, const char *what0, const char *what1, View *x1)
    {
        const int c1 = g.c[1], c2 = g.c[2];
        const rva_conv_weights *b0 = take(3, c1, k0, 2, what0), *b1 = take(c1, c2, 3, 2, what1);
        if (!b0 || !b1) return false;
        if (!b0->weight) return fail("b0: no stem convolution");
        Step s{}; s.H = g.H; s.W = g.W;
        if (p->f32) {                     // rva_stem_conv_f32: the checkpoint's [c1][3][3][3] weights as they are
            std::vector<float> sb(c1, 0.f);
            if (b0->bias) memcpy(sb.data(), b0->bias, sizeof(float) * c1);
            if (!upload(b0->weight, sizeof(float) * c1 * 27, sb, &s.w, &s.b)) return false;
        } else {
            // [64][128] fp16 in the checkpoint's own (c, ky, kx) order (6x6), or [64][32] fp16 in the column order k = 2 j + kx
            // (kx in {0, 1}), k = 18 + j (kx = 2), j = c*3 + ky (3x3); zero-padded
            if (c1 > 64) return fail("stem wider than 64 channels");
            const int cols = k0 == 6 ? 128 : 32;
            std::vector<_Float16> sw(64 * cols, (_Float16)0.f);
            std::vector<float> sb(64, 0.f);
            for (int co = 0; co < c1; ++co) {
                for (int k = 0; k < 3 * k0 * k0; ++k) {
                    const int j = k / 3, kx = k % 3;           // 3x3: weight[co][c][ky][kx] at k = 3 j + kx
                    sw[co * cols + (k0 == 6 ? k : kx < 2 ? 2 * j + kx : 18 + j)] = (_Float16)b0->weight[(size_t)co * 3 * k0 * k0 + k];
                }
                if (b0->bias) sb[co] = b0->bias[co];
            }
            if (!upload(sw.data(), sw.size() * 2, sb, &s.w, &s.b, k0 == 6 ? "weight" : "stem")) return false;
        }
        *x1 = buf(2, c2);
        p->fused_stem = !p->f32 && k0 == 3 && c1 == 32 && c2 == 64 && !(p->d.flags & RVA_PLAN_NO_STEM2);
        if (p->fused_stem) {              // both convolutions in one launch (rva_stem2_f16)
            s.kind = K_STEM2; s.out = x1->ptr(); s.ldo = x1->ld;
            if (!pack(&b1, 1, s, true)) return false;
            push(s, nullptr);
            return true;
        }
        View x0 = buf(1, c1);
        s.kind = p->f32 ? K_STEM_F32 : k0 == 6 ? K_STEM6 : K_STEM; s.out = x0.ptr(); s.ldo = x0.ld; s.Cout = c1;
        push(s, nullptr);
        return conv1(b1, x0, *x1, 1, 1);
    }
    // The backbone behind the stem: block 0 at level 2 into x2, then three times a 3x3 s2 and a block (into p3, p4 and a buffer of
    // level 5), and SPPF into p5.  what: the seven names b2 .. b8.  From the last 3x3 s2 on the pass is in its stride-32 phase.
    template <typename Block>
    bool backbone(Block block, View x, View x2, View p3, View p4, View p5, const char *const what[7])
    {
        const View dst[4] = {x2, p3, p4, buf(5, g.c[5])};
        for (int i = 0; i < 4; ++i) {
            if (i) {
                if (i == 3) p->quiet_step = (int)p->steps.size();
                View t = buf(2 + i, g.c[2 + i]);
                if (!conv1(take(x.ch, t.ch, 3, 2, what[2 * i - 1]), x, t, 1 + i, 1)) return false;
                x = t;
            }
            if (!block(i, x, dst[i], 2 + i, what[2 * i])) return false;
            x = dst[i];
        }
        return sppf(x, p5);
    }
    // FPN top-down path: n4 = block 4(cat[up(p5), p4]) and n3 = block 5(cat[up(n4), p3]), where cat4 = [. | p4] and cat3 = [. | p3]
    // are the concat buffers of level 4 and 3.  Upsample + concat are folded into the blocks' first 1x1 (conv_in) where every part
    // is a multiple of 64 channels wide; else an upsampling step fills the front of the concat buffer and the block reads it whole.
    template <typename Block>
    bool top_down(Block block, View p5, View cat4, View cat3, View n4, View n3, const char *what4, const char *what3)
    {
        const View p4 = cat4.sub(p5.ch, cat4.ch - p5.ch), p3 = cat3.sub(n4.ch, cat3.ch - n4.ch);
        const bool fuse_up = !p->f32 && p5.ch % 64 == 0 && p4.ch % 64 == 0 && n4.ch % 64 == 0 && p3.ch % 64 == 0 && g.h[4] == 2 * g.h[5] &&
                             g.w[4] == 2 * g.w[5] && g.h[3] == 2 * g.h[4] && g.w[3] == 2 * g.w[4];
        if (fuse_up) return block(4, Src(p5, p4), n4, 4, what4) && block(5, Src(n4, p3), n3, 3, what3);
        up2(p5, cat4.sub(0, p5.ch), 5);
        if (!block(4, cat4, n4, 4, what4)) return false;
        up2(n4, cat3.sub(0, n4.ch), 4);
        return block(5, cat3, n3, 3, what3);
    }
    // PAN bottom-up path: a 3x3 s2 of n3 into the front of cat4, m4 = block 6(cat4), a 3x3 s2 of m4 into the front of cat5,
    // m5 = block 7(cat5).  what: the four names in this order.  feats = {n3, m4, m5}: what the detect head reads.
    template <typename Block>
    bool bottom_up(Block block, View n3, View cat4, View cat5, View feats[3], const char *const what[4])
    {
        const View cat[2] = {cat4, cat5};
        feats[0] = n3; feats[1] = buf(4, g.c[4]); feats[2] = buf(5, g.c[5]);
        for (int i = 0; i < 2; ++i) {
            const View x = feats[i];
            fork_at[i] = (int)p->steps.size();             // x is complete here: its detect branch may start
            if (!conv1(take(x.ch, x.ch, 3, 2, what[2 * i]), x, cat[i].sub(0, x.ch), 3 + i, 1)) return false;
            if (!block(6 + i, cat[i], feats[i + 1], 4 + i, what[2 * i + 1])) return false;
        }
        return true;
    }
    // Detect head of YOLOv8 / YOLO11, opening: the widths, the anchors, whether the decode is fused into the last 1x1s, and the box
    // branches' convolutions (module order: all box branches first, then all class branches).  The class branch runs with its
    // interior width a multiple of 8 (16 where an fp32 convolution reads it) and ncp logit columns.
    bool head_open(Head &hd)
    {
        const int nc = p->d.nc, ncm = nc < 100 ? nc : 100, cal = p->f32 ? 16 : 8;
        hd.rm4 = 4 * p->d.reg_max;
        hd.cb = std::max(g.c[3] / 4, hd.rm4);
        hd.cc_real = std::max(g.c[3], ncm);
        hd.cc = (hd.cc_real + cal - 1) / cal * cal; hd.ncp = (nc + 7) / 8 * 8;
        hd.h3s = Step{}; hd.h3s.kind = K_HEAD3;
        p->A = g.a0(6);
        p->fused_head = !p->f32 && hd.cb % 64 == 0 && hd.cc % 64 == 0 && hd.rm4 == 64;
        for (int l = 0; l < 3; ++l) {
            hd.box[l][0] = take(g.c[3 + l], hd.cb, 3, 1, "detect.box.0"); hd.box[l][1] = take(hd.cb, hd.cb, 3, 1, "detect.box.1");
            hd.box[l][2] = take(hd.cb, hd.rm4, 1, 1, "detect.box.2");
            if (!hd.box[l][0] || !hd.box[l][1] || !hd.box[l][2]) return false;
        }
        return true;
    }
    // The last 1x1 of a detect branch at level l (mode 1: box, then mode 2: class): convolution + decode in one launch (fused head), or
    // the convolution into a buffer of its own that a decode step reads -- in an fp32 plan the level's own (rva_yolo_head_f32, on the
    // level's lane, behind its class branch), else the one step over all levels that head_close() pushes
    bool head_last(Head &hd, int l, int mode, const rva_conv_weights *c, View src)
    {
        if (p->fused_head) return head(c, src, mode, l);
        View o = buf(l, mode == 1 ? hd.rm4 : hd.ncp);
        if (!conv1(c, src, o, l, 0)) return false;
        Step &h = hd.h3s;
        const int i = l - 3;
        (mode == 1 ? h.hb : h.hk)[i] = o.ptr(); (mode == 1 ? h.hldb : h.hldc)[i] = o.ld; h.hh[i] = g.h[l]; h.hw[i] = g.w[l]; h.hs[i] = g.stride(l);
        if (p->f32 && mode == 2) {
            Step s{}; s.kind = K_HEAD_F32; s.in = h.hb[i]; s.ldi = h.hldb[i]; s.in2 = h.hk[i]; s.ldi2 = h.hldc[i];
            s.H = g.h[l]; s.W = g.w[l]; s.a0 = g.a0(l); s.stride_px = g.stride(l);
            push(s, nullptr);
        }
        return true;
    }
    bool head_close(Head &hd)
    {
        lane = 0;
        if (!p->fused_head && !p->f32) push(hd.h3s, nullptr);
        return err.empty();
    }

    // ---------------------------------------------------------------------------------------------- the three graphs
    bool build()
    {
        const rva_yolov8_desc &d = p->d;
        const int c3 = g.c[3], c4 = g.c[4], c5 = g.c[5];
        auto block = [&](int i, const Src &src, View dst, int l, const char *what) {
            const bool shortcut = i < 4;
            return c2f(dst.ch / 2, shortcut ? d.depth_backbone[i] : d.depth_head, src, dst, l, what,
                       [&](View x, View y) { return pair(x, y, shortcut, l, what); });
        };
        static const char *const backbone_names[7] = {"b2", "b3", "b4", "b5", "b6", "b7", "b8"}, *const up_names[4] = {"h16", "h18", "h19", "h21"};
        // concat buffers of the neck: producers write their slice directly
        View cat12 = buf(4, c5 + c4), cat15 = buf(3, c4 + c3), cat18 = buf(4, c3 + c4), cat21 = buf(5, c4 + c5);      // [up(p5) | p4], [up(n4) | p3], [h16 | n4], [h19 | p5]
        View p4 = cat12.sub(c5, c4), p3 = cat15.sub(c4, c3), n4 = cat18.sub(c3, c4), p5 = cat21.sub(c4, c5), n3 = buf(3, c3), x1, feats[3];
        if (!stem(3, "b0", "b1", &x1) || !backbone(block, x1, buf(2, g.c[2]), p3, p4, p5, backbone_names) ||
            !top_down(block, p5, cat12, cat15, n4, n3, "h12", "h15") || !bottom_up(block, n3, cat18, cat21, feats, up_names)) return false;
        // detect: per level one sibling launch for the first 3x3 of both branches (Cout = cb + cc), then each branch's 3x3 and last 1x1
        Head hd;
        if (!head_open(hd)) return false;
        const int cb = hd.cb, cc = hd.cc;
        const rva_conv_weights *cls[3][3];
        for (int l = 0; l < 3; ++l) {
            cls[l][0] = take(g.c[3 + l], hd.cc_real, 3, 1, "detect.cls.0"); cls[l][1] = take(hd.cc_real, hd.cc_real, 3, 1, "detect.cls.1");
            cls[l][2] = take(hd.cc_real, d.nc, 1, 1, "detect.cls.2");
            if (!cls[l][0] || !cls[l][1] || !cls[l][2]) return false;
            cls[l][0] = padded(cls[l][0], g.c[3 + l], cc); cls[l][1] = padded(cls[l][1], cc, cc); cls[l][2] = padded(cls[l][2], cc, hd.ncp);
        }
        if (!all_taken()) return false;
        for (int l = 0; l < 3; ++l) {
            // the three detect branches only depend on their own feature map and write disjoint anchor ranges: the stride-8 and
            // stride-16 branches may run on side streams beside the rest of the neck (rva_yolov8_plan_run_lanes)
            lane = ((p->fused_head || p->f32) && l < 2) ? l + 1 : 0;
            if (lane) p->fork_step[lane] = fork_at[l];
            View first = buf(3 + l, cb + cc), b2 = buf(3 + l, cb), k2 = buf(3 + l, cc);
            const rva_conv_weights *sib[2] = {hd.box[l][0], cls[l][0]};
            if (!conv(sib, 2, feats[l], first, 3 + l, 1)) return false;
            if (!conv1(hd.box[l][1], first.sub(0, cb), b2, 3 + l, 1) || !head_last(hd, 3 + l, 1, hd.box[l][2], b2)) return false;
            if (!conv1(cls[l][1], first.sub(cb, cc), k2, 3 + l, 1) || !head_last(hd, 3 + l, 2, cls[l][2], k2)) return false;
        }
        return head_close(hd);
    }

    bool build_v5(const float *anchors)
    {
        const rva_yolov8_desc &d = p->d;
        const int c3w = g.c[3], c4 = g.c[4], c5 = g.c[5];
        if (c3w % 64 || c4 % 64 || c5 % 64) return fail("YOLOv5 plan: c3, c4 and c5 must be multiples of 64 (the upsample + concat and head kernels)");
        auto block = [&](int i, const Src &src, View dst, int l, const char *what) {
            return c3(i < 4 ? d.depth_backbone[i] : d.depth_head, i < 4, src, dst, l, what);
        };
        static const char *const backbone_names[7] = {"b2", "b3", "b4", "b5", "b6", "b7", "b8"}, *const up_names[4] = {"h18", "h20", "h21", "h23"};
        // the two concat buffers of the bottom-up path; h14 / h10 write their slices directly
        View cat20 = buf(4, 2 * c3w), cat23 = buf(5, 2 * c4), t14 = cat20.sub(c3w, c3w), t10 = cat23.sub(c4, c4);
        View p3 = buf(3, c3w), p4 = buf(4, c4), p5 = buf(5, c5), n4 = buf(4, c4), n3 = buf(3, c3w), x1, feats[3];
        if (!stem(6, "b0", "b1", &x1) || !backbone(block, x1, buf(2, g.c[2]), p3, p4, p5, backbone_names)) return false;
        // top-down: a 1x1 in front of each upsampling, which is always folded into the block behind it
        if (!conv1(take(c5, c4, 1, 1, "h10"), p5, t10, 5, 1) || !block(4, Src(t10, p4), n4, 4, "h13") ||
            !conv1(take(c4, c3w, 1, 1, "h14"), n4, t14, 4, 1) || !block(5, Src(t14, p3), n3, 3, "h17")) return false;
        if (!bottom_up(block, n3, cat20, cat23, feats, up_names)) return false;
        // detect: one fused convolution + decode per level (three anchors per cell), into disjoint anchor ranges of the output
        const int co_real = 3 * (5 + d.nc), co = (co_real + 7) / 8 * 8;
        p->A = 3 * g.a0(6);
        const void *danc = nullptr;
        if (!upload(anchors, sizeof(float) * 18, &danc)) return false;
        for (int l = 3; l <= 5; ++l) {
            const rva_conv_weights *hc = padded(take(g.c[l], co_real, 1, 1, "detect.m"), g.c[l], co);
            Step s{}; s.kind = K_HEAD5;
            if (!hc || !pack(&hc, 1, s)) return false;
            const View &f = feats[l - 3];
            s.in = f.ptr(); s.ldi = f.ld; s.H = g.h[l]; s.W = g.w[l]; s.a0 = 3 * g.a0(l); s.stride_px = g.stride(l);
            s.b2 = (const float *)danc + 6 * (l - 3);
            push(s, "head5:%d->%d k1s1 %dx%d", s.Cin, s.Cout, s.H, s.W);
        }
        return all_taken() && err.empty();
    }

    bool build_11(const rva_yolo11_desc &e)
    {
        const int c3w = g.c[3], c4 = g.c[4], c5 = g.c[5];
        // C3k2: a C2f of inner width c = a quarter (blocks 0, 1) or half of its output whose inner blocks are bottlenecks 3x3 c -> c/2,
        // 3x3 c/2 -> c, or with c3k a C3k at width c with two bottlenecks, which writes its cv3 into the outer concat slice
        auto block = [&](int i, const Src &src, View dst, int l, const char *what) {
            const int c = i < 2 ? dst.ch / 4 : dst.ch / 2;
            const bool shortcut = i < 4;
            if (e.repeats[i] < 1 || c % 16) return fail("a C3k2 block needs at least one inner block and an inner width that is a multiple of 16");
            return c2f(c, e.repeats[i], src, dst, l, what, [&](View x, View y) {
                return e.c3k[i] ? c3(2, shortcut, x, y, l, what, 3) : bottleneck(x, y, c / 2, shortcut, l, what);
            });
        };
        static const char *const backbone_names[7] = {"2", "3", "4", "5", "6", "7", "8"}, *const up_names[4] = {"17", "19", "20", "22"};
        // concat buffers of the neck: producers write their slice directly
        View cat13 = buf(4, c5 + c4), cat16 = buf(3, c4 + c4), cat19 = buf(4, c3w + c4), cat22 = buf(5, c4 + c5);      // [up(p5) | p4], [up(n4) | p3], [17 | n4], [20 | p5]
        View p4 = cat13.sub(c5, c4), p3 = cat16.sub(c4, c4), n4 = cat19.sub(c3w, c4), p5 = cat22.sub(c4, c5), t5 = buf(5, c5), n3 = buf(3, c3w), x1, feats[3];
        if (!stem(3, "0", "1", &x1) || !backbone(block, x1, buf(2, c3w), p3, p4, t5, backbone_names) || !c2psa(e.psa_blocks, e.psa_heads, t5, p5) ||
            !top_down(block, p5, cat13, cat16, n4, n3, "13", "16") || !bottom_up(block, n3, cat19, cat22, feats, up_names)) return false;
        // detect: the box branch is YOLOv8's; the class branch is dw3x3, 1x1, dw3x3, 1x1, 1x1 with its interior width rounded up to 8
        // (zero-extended weights: a pad channel is SiLU(0) = 0 through the depthwise steps and meets zero weights).  No lanes.
        Head hd;
        if (!head_open(hd)) return false;
        const int cb = hd.cb, cr = hd.cc_real, cc = hd.cc;
        const rva_conv_weights *cls[3][5];
        for (int l = 0; l < 3; ++l) {
            const int ch = g.c[3 + l];
            cls[l][0] = take(1, ch, 3, 1, "detect.cls.0.0"); cls[l][1] = take(ch, cr, 1, 1, "detect.cls.0.1");
            cls[l][2] = take(1, cr, 3, 1, "detect.cls.1.0"); cls[l][3] = take(cr, cr, 1, 1, "detect.cls.1.1");
            cls[l][4] = take(cr, p->d.nc, 1, 1, "detect.cls.2");
            for (int i = 0; i < 5; ++i)
                if (!cls[l][i]) return false;
            cls[l][1] = padded(cls[l][1], ch, cc); cls[l][2] = padded(cls[l][2], 1, cc); cls[l][3] = padded(cls[l][3], cc, cc);
            cls[l][4] = padded(cls[l][4], cc, hd.ncp);
        }
        if (!all_taken()) return false;
        for (int l = 0; l < 3; ++l) {
            const int L = 3 + l;
            const View &f = feats[l];
            View bb1 = buf(L, cb), bb2 = buf(L, cb), d1 = buf(L, f.ch), k1 = buf(L, cc), d2 = buf(L, cc), k2 = buf(L, cc);
            if (!conv1(hd.box[l][0], f, bb1, L, 1) || !conv1(hd.box[l][1], bb1, bb2, L, 1)) return false;
            if (!dwconv(cls[l][0], 0, f, d1, L, 1) || !conv1(cls[l][1], d1, k1, L, 1) || !dwconv(cls[l][2], 0, k1, d2, L, 1) ||
                !conv1(cls[l][3], d2, k2, L, 1)) return false;
            if (!head_last(hd, L, 1, hd.box[l][2], bb2) || !head_last(hd, L, 2, cls[l][4], k2)) return false;
        }
        return head_close(hd);
    }
};

// whether this step, run with this variant, can restrict its launch to a row window
bool step_takes_rows(const Step &s, int variant)
{
    if (s.kind == K_STEM2 || s.kind == K_STEM6) return true;
    return s.kind == K_CONV && rva_conv_variant_rows(variant, s.Cin, s.k, s.stride);
}

// n: the leading images of every buffer the launch covers (the boxes32 side tensor stays where the capacity puts it).
// win: launch the step's row window where its kernel takes one (a primed plan; the tuner), else all rows
int launch_step(rva_yolov8_plan *p, const Step &s, int variant, const void *input, void *output, int n, rva_stream_t st, bool win)
{
    rva_ctx *c = p->ctx;
    if (win && (s.y0 > 0 || s.y1 < s.Ho) && step_takes_rows(s, variant)) {
        if (s.kind == K_STEM2) return rva_stem2_f16_rows(c, input, s.w, s.b, s.w2, s.b2, s.out, s.ldo, n, s.H, s.W, s.y0, s.y1, st);
        if (s.kind == K_STEM6) return rva_stem6_conv_f16_rows(c, input, s.w, s.b, s.out, s.ldo, n, s.H, s.W, s.Cout, s.y0, s.y1, st);
        return rva_conv2d_nhwc_f16_sel(c, s.in, s.ldi, s.w, s.b, s.out, s.ldo, s.res, s.ldr, n, p->B, s.H, s.W, s.Cin, s.Cout, s.k, s.stride, s.act,
                                       variant, s.y0, s.y1, st);
    }
    // the two launch forms that write box rows take the side tensor of this output (RVA_PLAN_BOX_F32), else none
    float *boxes = p->box32 && output ? (float *)((char *)output + p->box_off) : nullptr;
    switch (s.kind) {
    case K_CONV: return rva_conv2d_nhwc_f16_sel(c, s.in, s.ldi, s.w, s.b, s.out, s.ldo, s.res, s.ldr, n, p->B, s.H, s.W, s.Cin, s.Cout, s.k, s.stride, s.act, variant,
                                                0, -1, st);     // variant 0 chooses as for the capacity
    case K_UPCAT: return rva_conv1x1_upcat_f16(c, s.in, s.ldi, s.c_in, s.in2, s.ldi2, s.c_in2, s.w, s.b, s.out, s.ldo, n, s.H, s.W, s.Cout, s.act, variant, st);
    case K_HEAD: return rva_conv1x1_head_nc_f16(c, s.in, s.ldi, s.w, s.b, n, s.H, s.W, s.Cin, s.Cout, s.mode, output, s.mode == 1 ? boxes : nullptr, p->nc,
                                                p->A, s.a0, s.stride_px, variant, st);
    case K_PAIR32: return rva_c2f_pair32_f16(c, s.in, s.ldi, s.w, s.b, s.w2, s.b2, s.out, s.ldo, n, s.H, s.W, st);
    case K_STEM2: return rva_stem2_f16(c, input, s.w, s.b, s.w2, s.b2, s.out, s.ldo, n, s.H, s.W, st);
    case K_STEM: return rva_stem_conv_f16(c, input, s.w, s.b, s.out, s.ldo, n, s.H, s.W, s.Cout, st);
    case K_SPPF3: return rva_sppf_pool3_nhwc_f16(c, s.in, s.ldi, s.out, s.out2, s.out3, s.ldo, n, s.H, s.W, s.Cin, st);
    case K_POOL5: return rva_maxpool5_nhwc_f16(c, s.in, s.ldi, s.out, s.ldo, n, s.H, s.W, s.Cin, st);
    case K_UP2: return rva_upsample2x_nhwc_f16(c, s.in, s.ldi, s.out, s.ldo, n, s.H, s.W, s.Cin, st);
    case K_HEAD3: return rva_yolo_head3_nc_f16(c, s.hb, s.hldb, s.hk, s.hldc, output, boxes, n, s.hh, s.hw, p->nc, p->A, s.hs, st);
    case K_CONV_F32: return rva_conv2d_nhwc_f32_v(c, s.in, s.ldi, s.w, s.b, s.out, s.ldo, s.res, s.ldr, n, s.H, s.W, s.Cin, s.Cout, s.k, s.stride, s.act, variant, st);
    case K_STEM_F32: return rva_stem_conv_f32(c, input, s.w, s.b, s.out, s.ldo, n, s.H, s.W, s.Cout, st);
    case K_POOL5_F32: return rva_maxpool5_nhwc_f32(c, s.in, s.ldi, s.out, s.ldo, n, s.H, s.W, s.Cin, st);
    case K_UP2_F32: return rva_upsample2x_nhwc_f32(c, s.in, s.ldi, s.out, s.ldo, n, s.H, s.W, s.Cin, st);
    case K_STEM6: return rva_stem6_conv_f16(c, input, s.w, s.b, s.out, s.ldo, n, s.H, s.W, s.Cout, st);
    case K_HEAD5: return rva_conv1x1_head5_f16(c, s.in, s.ldi, s.w, s.b, n, s.H, s.W, s.Cin, p->nc, s.b2, output, boxes, p->A, s.a0, s.stride_px, variant, st);
    case K_HEAD_F32: return rva_yolo_head_f32(c, s.in, s.ldi, s.in2, s.ldi2, output, n, s.H, s.W, p->nc, p->A, s.a0, s.stride_px, st);
    case K_DWCONV: return rva_dwconv3x3_nhwc_f16(c, s.in, s.ldi, s.w, s.b, s.out, s.ldo, s.res, s.ldr, n, s.H, s.W, s.Cin, s.act, st);
    case K_ATTN: return rva_psa_attention_f16(c, s.in, s.ldi, s.out, s.ldo, n, s.H * s.W, s.mode, st);      // mode = heads
    }
    return RVA_ERR_ARG;
}

bool variant_fits(const Step &s, int variant)
{
    if (s.kind == K_CONV) return variant >= 0;
    if (s.kind == K_CONV_F32) return variant >= 0 && variant <= rva_conv_f32_num_variants();
    return variant == 0 || rva_conv_variant_is_gather64(variant);     // upcat / head: the LDS-DMA gather family
}

int out_rows(int H, int k, int stride) { return (H + 2 * (k / 2) - k) / stride + 1; }

// Windows of every step from the input window [top, bottom).  A written channel slice is known by the address of its first
// pixel; a reader takes the union over the slices its channels overlap, and the whole image for channels nobody registered
// (the outputs of the pooling / upsampling / head steps: those steps always run all rows).
void propagate_rows(rva_yolov8_plan *p)
{
    struct Slice { const char *lo, *hi; int H, y0, y1; };
    std::vector<Slice> written;
    const int es = p->f32 ? 4 : 2;
    const bool off = p->f32 || (p->rows_top <= 0 && p->rows_bottom >= p->H);
    // window of rows [*lo, *hi) of an H-row image read through `ptr`, `ch` channels wide: false = everything
    auto read = [&](const void *ptr, int ch, int H, int *lo, int *hi) {
        const char *a = (const char *)ptr, *b = a + (size_t)ch * es;
        long covered = 0;
        int y0 = H, y1 = 0;
        for (const Slice &w : written) {
            const char *l = w.lo > a ? w.lo : a, *h = w.hi < b ? w.hi : b;
            if (l >= h) continue;
            if (w.H != H) return false;
            covered += h - l;
            if (w.y0 < y0) y0 = w.y0;
            if (w.y1 > y1) y1 = w.y1;
        }
        if (covered != b - a || y0 >= y1) return false;
        *lo = y0; *hi = y1;
        return true;
    };
    auto through = [](int k, int stride, int H, int *lo, int *hi) {      // in place; returns the output height
        int32_t a = 0, b = 0;
        (void)rva_conv_rows_through(k, stride, H, *lo, *hi, &a, &b);
        *lo = a; *hi = b;
        return out_rows(H, k, stride);
    };
    p->windowed = false;
    for (Step &s : p->steps) {
        int lo = 0, hi = 0, Ho = s.H;
        bool known = false;
        switch (s.kind) {
        case K_STEM2: case K_STEM:
            lo = p->rows_top; hi = p->rows_bottom; known = true;
            Ho = through(3, 2, s.H, &lo, &hi);
            if (s.kind == K_STEM2) Ho = through(3, 2, Ho, &lo, &hi);
            break;
        case K_STEM6: {
            int32_t a = 0, b = 0;
            (void)rva_conv_rows_through_pad(6, 2, 2, s.H, p->rows_top, p->rows_bottom, &a, &b);
            lo = a; hi = b; known = true; Ho = s.H / 2;
            break;
        }
        case K_CONV:
            known = read(s.in, s.c_real, s.H, &lo, &hi);
            Ho = out_rows(s.H, s.k, s.stride);
            if (known) {
                (void)through(s.k, s.stride, s.H, &lo, &hi);
                int rl = 0, rh = 0;
                if (s.res) {                                   // the shortcut is added row for row
                    known = read(s.res, s.Cout, Ho, &rl, &rh);
                    if (rl < lo) lo = rl;
                    if (rh > hi) hi = rh;
                }
            }
            break;
        case K_PAIR32:
            known = read(s.in, 32, s.H, &lo, &hi);
            if (known) { (void)through(3, 1, s.H, &lo, &hi); (void)through(3, 1, s.H, &lo, &hi); }
            break;
        case K_UPCAT: {
            int l2 = 0, h2 = 0;
            known = read(s.in, s.c_in, s.H / 2, &lo, &hi) && read(s.in2, s.c_in2, s.H, &l2, &h2);
            lo = 2 * lo < l2 ? 2 * lo : l2;                    // low-resolution row r is rows 2r and 2r + 1 here
            hi = 2 * hi > h2 ? 2 * hi : h2;
            break;
        }
        default: break;
        }
        s.Ho = Ho;
        if (off || !known || lo >= hi) { lo = 0; hi = Ho; }
        s.y0 = lo; s.y1 = hi;
        if (lo > 0 || hi < Ho) p->windowed = true;
        if (s.kind == K_STEM2 || s.kind == K_STEM || s.kind == K_STEM6 || s.kind == K_CONV || s.kind == K_PAIR32 || s.kind == K_UPCAT) {
            const int ch = s.kind == K_STEM2 ? 64 : s.kind == K_PAIR32 ? 32 : s.Cout;
            written.push_back(Slice{(const char *)s.out, (const char *)s.out + (size_t)ch * es, Ho, lo, hi});
        }
    }
    for (Tunable &t : p->tunables) {
        const Step &s = p->steps[t.step];
        t.desc = t.base;
        if (s.y0 > 0 || s.y1 < s.Ho) {
            char w[32];
            snprintf(w, sizeof w, " r[%d,%d)", s.y0, s.y1);
            t.desc += w;
        }
    }
    p->primed = 0;
}

bool stream_is_capturing(rva_stream_t stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

int run_steps(rva_yolov8_plan *p, const void *input, void *output, int n, int first, int last, rva_stream_t stream, bool win)
{
    for (int i = first; i < last; ++i) {
        const Step &s = p->steps[i];
        const int rc = launch_step(p, s, s.variant, input, output, n, stream, win);
        if (rc != RVA_OK) return rc;
    }
    return RVA_OK;
}

// what every run entry point refuses before it launches anything
int check_run(rva_yolov8_plan *p, const void *input, void *output, int n)
{
    if (!p || !input || !output) return RVA_ERR_ARG;
    if (n <= 0 || n > p->B) return rva_fail(p->ctx, RVA_ERR_ARG, "rva_yolov8_plan_run: n = %d is not 1 .. %d, the plan's capacity", n, p->B);
    if (((uintptr_t)input | (uintptr_t)output) % 16) return rva_fail(p->ctx, RVA_ERR_ARG, "rva_yolov8_plan_run: input and output must be 16-byte aligned");
    return RVA_OK;
}

// A whole run over all rows of n images has been queued: later runs of up to n images may launch windows.  A run that is only
// recorded (stream capture) executes who knows when, or never: it leaves the count alone.
void note_complete_run(rva_yolov8_plan *p, int n, bool win, rva_stream_t stream)
{
    if (!win && !stream_is_capturing(stream)) p->primed = n;
}

// The internal descriptor from the fields every public descriptor has (reg_max 16: what the plan runs with)
template <typename D>
rva_yolov8_desc internal_desc(const D &e)
{
    rva_yolov8_desc d{};
    d.batch = e.batch; d.height = e.height; d.width = e.width; d.nc = e.nc; d.reg_max = 16; d.n_convs = e.n_convs; d.flags = e.flags;
    memcpy(d.widths, e.widths, sizeof d.widths);
    return d;
}

struct PlanDeleter { void operator()(rva_yolov8_plan *p) const { rva_yolov8_plan_destroy(p); } };

// What the create entry points share.  `d`: the internal descriptor the entry filled; `also`: what its rule adds to the common
// one; `refuse()`: the architecture's own refusals (RVA_OK: none); `build(builder)`: the graph to lay down.  The plan under
// construction is held so that every return releases its device allocations and events, as rva_yolov8_plan_destroy does.
template <typename Refuse, typename Build>
int create_plan(rva_ctx *ctx, const char *who, const char *also, const rva_yolov8_desc &d, int head_rows, const rva_conv_weights *convs,
                rva_yolov8_plan **out, Refuse refuse, Build build)
{
    *out = nullptr;
    if (d.batch <= 0 || d.height <= 0 || d.width <= 0 || d.height % 32 || d.width % 32 || d.nc < 1 || d.nc > 1024 || d.reg_max != 16 || d.n_convs <= 0)
        return rva_fail(ctx, RVA_ERR_ARG, "%s: batch > 0, height and width multiples of 32, 1 <= nc <= 1024%s", who, also);
    for (int i = 0; i < 5; ++i)
        if (d.widths[i] <= 0 || d.widths[i] % 8) return rva_fail(ctx, RVA_ERR_ARG, "%s: channel widths must be multiples of 8", who);
    if (const int rc = refuse(); rc != RVA_OK) return rc;
    RVA_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<rva_yolov8_plan, PlanDeleter> p(new rva_yolov8_plan());
    p->ctx = ctx; p->d = d; p->B = d.batch; p->H = d.height; p->W = d.width; p->nc = d.nc;
    p->head_rows = head_rows;
    p->f32 = (d.flags & RVA_PLAN_F32) != 0;
    p->box32 = (d.flags & RVA_PLAN_BOX_F32) != 0;
    Builder b(p.get(), convs);
    if (!build(b)) return rva_fail(ctx, b.hip_failed ? RVA_ERR_HIP : RVA_ERR_ARG, "%s: %s", who, b.err.c_str());
    for (int l = 1; l <= 2; ++l)
        if (p->fork_step[l] >= 0) {
            RVA_HIP(ctx, hipEventCreateWithFlags(&p->fork_ev[l], hipEventDisableTiming));
            RVA_HIP(ctx, hipEventCreateWithFlags(&p->join_ev[l], hipEventDisableTiming));
        }
    RVA_HIP(ctx, hipDeviceSynchronize());                  // weights are in place before the first run on any stream
    if (p->box32) p->box_off = ((size_t)p->B * p->head_rows * p->A * 2 + 255) / 256 * 256;
    p->rows_top = 0; p->rows_bottom = p->H;
    propagate_rows(p.get());
    *out = p.release();
    return RVA_OK;
}

}  // namespace

extern "C" {

int rva_yolov8_plan_create(rva_ctx *ctx, const rva_yolov8_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out)
{
    if (!ctx || !desc || !convs || !out) return RVA_ERR_ARG;
    const char *who = "rva_yolov8_plan_create";
    return create_plan(ctx, who, ", reg_max 16", *desc, 4 + desc->nc, convs, out, [&] {
        if ((desc->flags & RVA_PLAN_F32) && (desc->flags & RVA_PLAN_BOX_F32))
            return rva_fail(ctx, RVA_ERR_ARG, "%s: RVA_PLAN_BOX_F32 belongs to fp16 plans (the output of an RVA_PLAN_F32 plan is fp32 already)", who);
        return (int)RVA_OK;
    }, [](Builder &b) { return b.build(); });
}

int rva_yolov5_plan_create(rva_ctx *ctx, const rva_yolov5_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out)
{
    if (!ctx || !desc || !convs || !out) return RVA_ERR_ARG;
    const char *who = "rva_yolov5_plan_create";
    rva_yolov8_desc d = internal_desc(*desc);
    memcpy(d.depth_backbone, desc->depth_backbone, sizeof d.depth_backbone);
    d.depth_head = desc->depth_head;
    return create_plan(ctx, who, "", d, 5 + desc->nc, convs, out, [&] {
        if (desc->flags & RVA_PLAN_F32) return rva_fail(ctx, RVA_ERR_ARG, "%s: there is no fp32 YOLOv5 plan (RVA_PLAN_F32); build the fp16 plan", who);
        for (int i = 0; i < 18; ++i)
            if (!(desc->anchors[i] > 0.f) || !(desc->anchors[i] < 65504.f)) return rva_fail(ctx, RVA_ERR_ARG, "%s: anchors must be positive pixel sizes", who);
        return (int)RVA_OK;
    }, [&](Builder &b) { return b.build_v5(desc->anchors); });
}

int rva_yolo11_plan_create(rva_ctx *ctx, const rva_yolo11_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out)
{
    if (!ctx || !desc || !convs || !out) return RVA_ERR_ARG;
    const char *who = "rva_yolo11_plan_create";
    return create_plan(ctx, who, "", internal_desc(*desc), 4 + desc->nc, convs, out, [&] {
        if (desc->flags & RVA_PLAN_F32) return rva_fail(ctx, RVA_ERR_ARG, "%s: there is no fp32 YOLO11 plan (RVA_PLAN_F32); build the fp16 plan", who);
        if (desc->psa_heads < 1 || desc->psa_heads * 128 != desc->widths[4])
            return rva_fail(ctx, RVA_ERR_ARG, "%s: psa_heads * 64 = %d is not half the C2PSA width %d", who, desc->psa_heads * 64, desc->widths[4]);
        return (int)RVA_OK;
    }, [&](Builder &b) { return b.build_11(*desc); });
}

void rva_yolov8_plan_destroy(rva_yolov8_plan *p)
{
    if (!p) return;
    for (void *a : p->allocs) (void)hipFree(a);
    for (int l = 0; l < 3; ++l) {
        if (p->fork_ev[l]) (void)hipEventDestroy(p->fork_ev[l]);
        if (p->join_ev[l]) (void)hipEventDestroy(p->join_ev[l]);
    }
    delete p;
}

int rva_yolov8_plan_info(const rva_yolov8_plan *p, int32_t *anchors, int32_t *out_rows, int32_t *n_steps, int32_t *n_tunable, int32_t *quiet_step)
{
    if (!p) return RVA_ERR_ARG;
    if (anchors) *anchors = p->A;
    if (out_rows) *out_rows = p->head_rows;
    if (n_steps) *n_steps = (int32_t)p->steps.size();
    if (n_tunable) *n_tunable = (int32_t)p->tunables.size();
    if (quiet_step) *quiet_step = p->quiet_step;
    return RVA_OK;
}

int rva_yolov8_plan_output_layout(const rva_yolov8_plan *p, int64_t *total_bytes, int64_t *boxes_offset)
{
    if (!p) return RVA_ERR_ARG;
    const size_t head = (size_t)p->B * p->head_rows * p->A * (p->f32 ? 4 : 2);
    if (total_bytes) *total_bytes = (int64_t)(p->box32 ? p->box_off + (size_t)p->B * 4 * p->A * 4 : head);
    if (boxes_offset) *boxes_offset = p->box32 ? (int64_t)p->box_off : -1;
    return RVA_OK;
}

int rva_yolov8_plan_tunable_desc(const rva_yolov8_plan *p, int index, char *buf, int len)
{
    if (!p || index < 0 || index >= (int)p->tunables.size() || !buf || len <= 0) return RVA_ERR_ARG;
    snprintf(buf, (size_t)len, "%s", p->tunables[index].desc.c_str());
    return RVA_OK;
}

// What step `step` of the list is: a tunable step's description, else the kernel's name and the shape it runs.
int rva_yolov8_plan_step_desc(const rva_yolov8_plan *p, int step, char *buf, int len)
{
    if (!p || step < 0 || step >= (int)p->steps.size() || !buf || len <= 0) return RVA_ERR_ARG;
    const Step &s = p->steps[step];
    if (s.tunable >= 0) { snprintf(buf, (size_t)len, "%s", p->tunables[s.tunable].desc.c_str()); return RVA_OK; }
    switch (s.kind) {
    case K_ATTN: snprintf(buf, (size_t)len, "attention heads %d tokens %d", s.mode, s.H * s.W); break;
    case K_DWCONV: snprintf(buf, (size_t)len, "dwconv3x3 %d act%d%s %dx%d", s.Cin, s.act, s.res ? " +res" : "", s.H, s.W); break;
    case K_STEM2: snprintf(buf, (size_t)len, "stem2 3->32->64 %dx%d", s.H, s.W); break;
    case K_STEM: case K_STEM_F32: snprintf(buf, (size_t)len, "stem 3->%d k3s2 %dx%d", s.Cout, s.H, s.W); break;
    case K_STEM6: snprintf(buf, (size_t)len, "stem6 3->%d k6s2 %dx%d", s.Cout, s.H, s.W); break;
    case K_PAIR32: snprintf(buf, (size_t)len, "pair32 %dx%d", s.H, s.W); break;
    case K_SPPF3: snprintf(buf, (size_t)len, "sppf pool3 %d %dx%d", s.Cin, s.H, s.W); break;
    case K_POOL5: case K_POOL5_F32: snprintf(buf, (size_t)len, "maxpool5 %d %dx%d", s.Cin, s.H, s.W); break;
    case K_UP2: case K_UP2_F32: snprintf(buf, (size_t)len, "upsample2x %d %dx%d", s.Cin, s.H, s.W); break;
    case K_HEAD3: snprintf(buf, (size_t)len, "head3 decode"); break;
    case K_HEAD_F32: snprintf(buf, (size_t)len, "head decode %dx%d", s.H, s.W); break;
    default: snprintf(buf, (size_t)len, "step kind %d", (int)s.kind); break;
    }
    return RVA_OK;
}

int rva_yolov8_plan_set_variant(rva_yolov8_plan *p, int index, int variant)
{
    if (!p || index < 0 || index >= (int)p->tunables.size()) return RVA_ERR_ARG;
    Step &s = p->steps[p->tunables[index].step];
    if (!variant_fits(s, variant) || variant > rva_conv_num_variants()) return rva_fail(p->ctx, RVA_ERR_ARG, "rva_yolov8_plan_set_variant: variant %d does not exist for this layer", variant);
    p->primed = 0;                                         // another kernel may cover other rows: one whole run first
    s.variant = variant;
    return RVA_OK;
}

int rva_yolov8_plan_get_variant(const rva_yolov8_plan *p, int index)
{
    if (!p || index < 0 || index >= (int)p->tunables.size()) return -1;
    return p->steps[p->tunables[index].step].variant;
}

int rva_yolov8_plan_launch_tunable(rva_yolov8_plan *p, int index, int variant, void *output, rva_stream_t stream)
{
    if (!p || index < 0 || index >= (int)p->tunables.size()) return RVA_ERR_ARG;
    const Step &s = p->steps[p->tunables[index].step];
    if (!variant_fits(s, variant)) return RVA_ERR_ARG;
    if ((s.kind == K_HEAD || s.kind == K_HEAD5) && !output) return RVA_ERR_ARG;
    return launch_step(p, s, variant, nullptr, output, p->B, stream, true);      // all images; the row window where the variant takes one: what a primed run launches
}

int rva_yolov8_plan_run_range_n(rva_yolov8_plan *p, const void *input, void *output, int n, int first, int last, rva_stream_t stream)
{
    if (const int rc = check_run(p, input, output, n); rc != RVA_OK) return rc;
    if (first < 0 || last > (int)p->steps.size() || first > last) return RVA_ERR_ARG;
    return run_steps(p, input, output, n, first, last, stream, n <= p->primed);       // a range never primes
}

int rva_yolov8_plan_run_range(rva_yolov8_plan *p, const void *input, void *output, int first, int last, rva_stream_t stream)
{
    return p ? rva_yolov8_plan_run_range_n(p, input, output, p->B, first, last, stream) : RVA_ERR_ARG;
}

int rva_yolov8_plan_run_n(rva_yolov8_plan *p, const void *input, void *output, int n, rva_stream_t stream)
{
    if (const int rc = check_run(p, input, output, n); rc != RVA_OK) return rc;
    const bool win = n <= p->primed;
    const int rc = run_steps(p, input, output, n, 0, (int)p->steps.size(), stream, win);
    if (rc == RVA_OK) note_complete_run(p, n, win, stream);
    return rc;
}

int rva_yolov8_plan_run(rva_yolov8_plan *p, const void *input, void *output, rva_stream_t stream)
{
    return p ? rva_yolov8_plan_run_n(p, input, output, p->B, stream) : RVA_ERR_ARG;
}

int rva_yolov8_plan_primed_images(const rva_yolov8_plan *p) { return p ? p->primed : 0; }

int rva_yolov8_plan_set_static_rows(rva_yolov8_plan *p, int top, int bottom)
{
    if (!p) return RVA_ERR_ARG;
    if (top < 0 || bottom > p->H || top >= bottom)
        return rva_fail(p->ctx, RVA_ERR_ARG, "rva_yolov8_plan_set_static_rows: [%d, %d) is not a window of %d rows", top, bottom, p->H);
    const char *e = getenv("RVA_PLAN_NO_STATIC_ROWS");
    if (e && e[0] == '1') return RVA_OK;                   // A/B switch: the plan stays un-windowed
    p->rows_top = top; p->rows_bottom = bottom;
    propagate_rows(p);                                     // (an fp32 plan keeps whole images)
    return RVA_OK;
}

int rva_yolov8_plan_step_rows(const rva_yolov8_plan *p, int step, int32_t *y0, int32_t *y1)
{
    if (!p || step < 0 || step >= (int)p->steps.size()) return RVA_ERR_ARG;
    if (y0) *y0 = p->steps[step].y0;
    if (y1) *y1 = p->steps[step].y1;
    return RVA_OK;
}

// Output rows of a k x k, pad k / 2 convolution that see an input row of [lo, hi): row o reads o * stride - k / 2 .. + k - 1
int rva_conv_rows_through(int k, int stride, int H_in, int lo, int hi, int32_t *out_lo, int32_t *out_hi)
{
    if ((k != 1 && k != 3) || (stride != 1 && stride != 2)) return RVA_ERR_ARG;
    return rva_conv_rows_through_pad(k, stride, k / 2, H_in, lo, hi, out_lo, out_hi);
}

// The same for any padding (the 6x6 stride-2 pad-2 stem of YOLOv5): row o reads o * stride - pad .. + k - 1
int rva_conv_rows_through_pad(int k, int stride, int pad, int H_in, int lo, int hi, int32_t *out_lo, int32_t *out_hi)
{
    if (k < 1 || stride < 1 || pad < 0 || pad >= k || H_in <= 0 || lo < 0 || hi > H_in || lo >= hi || !out_lo || !out_hi) return RVA_ERR_ARG;
    if (H_in + 2 * pad < k) return RVA_ERR_ARG;
    const int Ho = (H_in + 2 * pad - k) / stride + 1;
    // o * stride - pad + k - 1 >= lo  and  o * stride - pad <= hi - 1
    int a = lo + pad - (k - 1), b = hi - 1 + pad;
    a = a <= 0 ? 0 : (a + stride - 1) / stride;
    b = b / stride + 1;
    if (b > Ho) b = Ho;
    if (a > b) a = b;
    *out_lo = a; *out_hi = b;
    return RVA_OK;
}

int rva_yolov8_plan_run_lanes(rva_yolov8_plan *p, const void *input, void *output, rva_stream_t stream, rva_stream_t side1, rva_stream_t side2)
{
    return p ? rva_yolov8_plan_run_lanes_n(p, input, output, p->B, stream, side1, side2) : RVA_ERR_ARG;
}

int rva_yolov8_plan_run_lanes_n(rva_yolov8_plan *p, const void *input, void *output, int n, rva_stream_t stream, rva_stream_t side1, rva_stream_t side2)
{
    if (const int rc = check_run(p, input, output, n); rc != RVA_OK) return rc;
    if (!side1 || !side2 || p->fork_step[1] < 0) return rva_yolov8_plan_run_n(p, input, output, n, stream);
    hipStream_t lanes[3] = {(hipStream_t)stream, (hipStream_t)side1, (hipStream_t)side2};
    bool started[3] = {true, false, false};
    const bool win = n <= p->primed;
    for (int i = 0; i < (int)p->steps.size(); ++i) {
        for (int l = 1; l <= 2; ++l)
            if (p->fork_step[l] == i) RVA_HIP(p->ctx, hipEventRecord(p->fork_ev[l], lanes[0]));      // everything the main lane has been given so far
        const Step &s = p->steps[i];
        if (s.lane && !started[s.lane]) {
            RVA_HIP(p->ctx, hipStreamWaitEvent(lanes[s.lane], p->fork_ev[s.lane], 0));
            started[s.lane] = true;
        }
        const int rc = launch_step(p, s, s.variant, input, output, n, (rva_stream_t)lanes[s.lane], win);
        if (rc != RVA_OK) return rc;
    }
    for (int l = 1; l <= 2; ++l)
        if (started[l]) {
            RVA_HIP(p->ctx, hipEventRecord(p->join_ev[l], lanes[l]));
            RVA_HIP(p->ctx, hipStreamWaitEvent(lanes[0], p->join_ev[l], 0));
        }
    note_complete_run(p, n, win, stream);                  // as rva_yolov8_plan_run_n
    return RVA_OK;
}

}  // extern "C"
