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
// rva_yolov5_plan_create and rva_yolo11_plan_create lay down the graphs of YOLOv5 and YOLO11 for the same plan object
// (Builder::build_v5 / build_11; the graphs and module orders are in include/rva.h).  YOLO11 adds two step kinds, K_DWCONV and
// K_ATTN (rva_attn.hip): fixed kernels like the pooling steps, and in propagate_rows always the whole map -- attention is global.
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

struct Builder {
    rva_yolov8_plan *p;
    const rva_conv_weights *convs;
    int next = 0;                         // next convolution of the module-order list
    int lane = 0;
    std::string err;
    std::deque<std::vector<float>> pad_store;             // zero-extended host copies of the class branch (padded) ...
    std::deque<rva_conv_weights> pad_convs;               // ... and their descriptors

    bool fail(const std::string &m) { if (err.empty()) err = m; return false; }

    void *dev_alloc(size_t bytes, bool zero)
    {
        void *ptr = nullptr;
        if (hipMalloc(&ptr, bytes ? bytes : 16) != hipSuccess) { fail("hipMalloc failed"); return nullptr; }
        p->allocs.push_back(ptr);
        if (zero && hipMemset(ptr, 0, bytes) != hipSuccess) { fail("hipMemset failed"); return nullptr; }
        return ptr;
    }
    View buf(long m, int ch)
    {
        View v;
        // + 64 B: a convolution whose Cin is not a multiple of 32 runs with Cin rounded up (zero weights for the extra channels, see
        // conv()) and reads up to 31 channels past its slice -- the next slice of the row, the next row, or, behind the last row, this slack
        v.es = p->f32 ? 4 : 2;
        v.base = (char *)dev_alloc((size_t)m * ch * v.es + 64, true);
        v.ld = ch; v.off = 0; v.ch = ch;
        return v;
    }
    // Pack sibling convolutions (equal Cin / kernel / stride, outputs concatenated) as [CoutPad][k*k][CinPad] fp16 + [CoutPad] fp32
    bool upload(const void *host, size_t bytes, const void **dev)
    {
        void *d = dev_alloc(bytes, false);
        if (!d) return false;
        if (hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("weight upload failed");
        *dev = d;
        return true;
    }
    // fp32 plan: sibling convolutions packed as [Cout][k*k][Cin] fp32 (no padding: rva_conv2d_nhwc_f32_v masks the tile edges) + [Cout] fp32
    bool pack_f32(const rva_conv_weights *const *cv, int n, const void **w_dev, const float **b_dev, int *cin, int *cout, int *k, int *stride)
    {
        const rva_conv_weights &c0 = *cv[0];
        int co = 0;
        for (int i = 0; i < n; ++i) {
            if (!cv[i]->weight || cv[i]->cin != c0.cin || cv[i]->k != c0.k || cv[i]->stride != c0.stride) return fail("sibling convolutions differ");
            co += cv[i]->cout;
        }
        const int kk = c0.k * c0.k;
        std::vector<float> hw((size_t)co * kk * c0.cin, 0.f), hb(co, 0.f);
        int o = 0;
        for (int i = 0; i < n; ++i) {
            const rva_conv_weights &c = *cv[i];
            for (int oc = 0; oc < c.cout; ++oc) {
                for (int ic = 0; ic < c.cin; ++ic)
                    for (int t = 0; t < kk; ++t)
                        hw[((size_t)(o + oc) * kk + t) * c.cin + ic] = c.weight[((size_t)oc * c.cin + ic) * kk + t];
                if (c.bias) hb[o + oc] = c.bias[oc];
            }
            o += c.cout;
        }
        const void *db = nullptr;
        if (!upload(hw.data(), hw.size() * 4, w_dev) || !upload(hb.data(), hb.size() * 4, &db)) return false;
        *b_dev = (const float *)db; *cin = c0.cin; *cout = co; *k = c0.k; *stride = c0.stride;
        return true;
    }
    bool pack(const rva_conv_weights *const *cv, int n, const void **w_dev, const float **b_dev, int *cin, int *cout, int *k, int *stride)
    {
        const rva_conv_weights &c0 = *cv[0];
        int co = 0;
        for (int i = 0; i < n; ++i) {
            if (!cv[i]->weight || cv[i]->cin != c0.cin || cv[i]->k != c0.k || cv[i]->stride != c0.stride) return fail("sibling convolutions differ");
            co += cv[i]->cout;
        }
        const int kk = c0.k * c0.k, cpad = rva_conv_cout_pad(co), cinp = (c0.cin + 31) / 32 * 32;
        std::vector<_Float16> hw((size_t)cpad * kk * cinp, (_Float16)0.f);
        std::vector<float> hb(cpad, 0.f);
        int o = 0;
        for (int i = 0; i < n; ++i) {
            const rva_conv_weights &c = *cv[i];
            for (int oc = 0; oc < c.cout; ++oc) {
                for (int ic = 0; ic < c.cin; ++ic)
                    for (int t = 0; t < kk; ++t)
                        hw[((size_t)(o + oc) * kk + t) * cinp + ic] = (_Float16)c.weight[((size_t)oc * c.cin + ic) * kk + t];
                if (c.bias) hb[o + oc] = c.bias[oc];
            }
            o += c.cout;
        }
        void *dw = dev_alloc(hw.size() * 2, false), *db = dev_alloc(hb.size() * 4, false);
        if (!dw || !db) return false;
        if (hipMemcpy(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return fail("weight upload failed");
        *w_dev = dw; *b_dev = (const float *)db; *cin = c0.cin; *cout = co; *k = c0.k; *stride = c0.stride;
        return true;
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
    // one Conv-BN-SiLU (or a fused group of siblings); returns false on error
    bool conv(const rva_conv_weights *const *cv, int n, View src, View dst, int h, int w, int act, const View *res = nullptr)
    {
        Step s{}; s.kind = p->f32 ? K_CONV_F32 : K_CONV;
        const bool packed = p->f32 ? pack_f32(cv, n, &s.w, &s.b, &s.Cin, &s.Cout, &s.k, &s.stride)
                                   : pack(cv, n, &s.w, &s.b, &s.Cin, &s.Cout, &s.k, &s.stride);
        if (!packed) return false;
        if (s.Cin != src.ch || s.Cout != dst.ch) return fail("convolution does not fit its buffers");
        s.in = src.ptr(); s.ldi = src.ld; s.out = dst.ptr(); s.ldo = dst.ld; s.H = h; s.W = w; s.act = act;
        if (res) { s.res = res->ptr(); s.ldr = res->ld; }
        const int cin_real = s.Cin;
        s.c_real = cin_real;
        if (p->f32) {                     // every channel count is read as it is: the kernel never reads past its slice
            if (s.Cin % 16) return fail("fp32 plan: convolution input channels must be multiples of 16");
            push(s, "%d->%d k%ds%d %dx%d", cin_real, s.Cout, s.k, s.stride, h, w);
            return true;
        }
        // Cin 48 / 16 (YOLOv8m / n): the LDS-DMA kernels want whole 32-channel chunks.  The packed weights already carry zero
        // columns up to the next multiple of 32, so the step simply declares the padded Cin: the extra channels it reads are whatever
        // follows the slice (finite activations of the neighbouring slice / pixel, or the buffer's zero slack) times zero.
        if (s.Cin % 32 && !(p->d.flags & RVA_PLAN_NO_CIN_PAD)) s.Cin = (s.Cin + 31) / 32 * 32;
        push(s, "%d->%d k%ds%d %dx%d", cin_real, s.Cout, s.k, s.stride, h, w);
        return true;
    }
    bool conv1(const rva_conv_weights *c, View src, View dst, int h, int w, int act, const View *res = nullptr)
    {
        return c && conv(&c, 1, src, dst, h, w, act, res);
    }
    bool upcat(const rva_conv_weights *c, View low, View skip, View dst, int h, int w) { return c && upcat(&c, 1, low, skip, dst, h, w); }
    bool upcat(const rva_conv_weights *const *cv, int n, View low, View skip, View dst, int h, int w)
    {
        Step s{}; s.kind = K_UPCAT;
        if (!pack(cv, n, &s.w, &s.b, &s.Cin, &s.Cout, &s.k, &s.stride)) return false;
        if (s.k != 1 || s.stride != 1 || s.Cin != low.ch + skip.ch || s.Cout != dst.ch) return fail("upsample + concat convolution does not fit");
        s.in = low.ptr(); s.ldi = low.ld; s.c_in = low.ch; s.in2 = skip.ptr(); s.ldi2 = skip.ld; s.c_in2 = skip.ch;
        s.out = dst.ptr(); s.ldo = dst.ld; s.H = h; s.W = w; s.act = 1;
        push(s, "up%d+%d->%d k1s1 %dx%d", low.ch, skip.ch, s.Cout, h, w);
        return true;
    }
    bool head(const rva_conv_weights *c, View src, int mode, int h, int w, int a0, float stride_px)
    {
        if (!c) return false;
        Step s{}; s.kind = K_HEAD;
        if (!pack(&c, 1, &s.w, &s.b, &s.Cin, &s.Cout, &s.k, &s.stride)) return false;
        if (s.k != 1 || s.stride != 1 || s.Cin != src.ch) return fail("head convolution does not fit");
        s.in = src.ptr(); s.ldi = src.ld; s.H = h; s.W = w; s.mode = mode; s.a0 = a0; s.stride_px = stride_px;
        push(s, "head%d:%d->%d k1s1 %dx%d", mode, s.Cin, s.Cout, h, w);
        return true;
    }
    // C2f: src is one view, or (low, skip) standing for cat([upsample2x(low), skip])
    bool c2f(int c1, int c2, int n, bool shortcut, const View *src, const View *low, const View *skip, View dst, int h, int w, const char *what)
    {
        const int c = c2 / 2;
        const long m = (long)p->B * h * w;
        const rva_conv_weights *cv1 = take(c1, 2 * c, 1, 1, what), *cv2 = take((2 + n) * c, c2, 1, 1, what);
        if (!cv1 || !cv2) return false;
        View cat = buf(m, (2 + n) * c);
        if (!cat.base) return false;
        if (low) { if (!upcat(cv1, *low, *skip, cat.sub(0, 2 * c), h, w)) return false; }
        else if (!conv1(cv1, *src, cat.sub(0, 2 * c), h, w, 1)) return false;
        for (int i = 0; i < n; ++i) {
            const rva_conv_weights *b1 = take(c, c, 3, 1, what), *b2 = take(c, c, 3, 1, what);
            View x = cat.sub((1 + i) * c, c);
            if (c == 32 && shortcut && !p->f32 && !(p->d.flags & RVA_PLAN_NO_PAIR32)) {
                // both 3x3 convolutions and the shortcut in one launch, the intermediate in LDS (rva_c2f_pair32_f16)
                Step s{}; s.kind = K_PAIR32;
                int ci, co, kk, st;
                if (!pack(&b1, 1, &s.w, &s.b, &ci, &co, &kk, &st) || !pack(&b2, 1, &s.w2, &s.b2, &ci, &co, &kk, &st)) return false;
                View y = cat.sub((2 + i) * c, c);
                s.in = x.ptr(); s.ldi = x.ld; s.out = y.ptr(); s.ldo = y.ld; s.H = h; s.W = w; s.Cin = s.Cout = c; s.k = 3; s.stride = 1; s.act = 1;
                push(s, nullptr);
                continue;
            }
            // the intermediate, one buffer per bottleneck: with row windows a step rewrites part of its output only, and the rest must
            // still be what THIS bottleneck's first convolution left there (the second one reads it as halo)
            View tmp = buf(m, c);
            if (!tmp.base) return false;
            if (!conv1(b1, x, tmp, h, w, 1)) return false;
            if (!conv1(b2, tmp, cat.sub((2 + i) * c, c), h, w, 1, shortcut ? &x : nullptr)) return false;
        }
        return conv1(cv2, cat, dst, h, w, 1);
    }

    // YOLOv5's C3: src is one view, or (low, skip) standing for cat([upsample2x(low), skip]).  cv1 and cv2 read the same input:
    // one sibling launch writes cat[0, 2c) = [cv1 out | cv2 out]; the bottlenecks x <- x + cv2_3x3(cv1_1x1(x)) start from cv1 out,
    // the last one writes cat[2c, 3c), and cv3 reads cat[c, 3c) = [cv2 out | m out] with the halves of its input channels swapped
    // on the host (the module concatenates [m out | cv2 out]).
    // k1: kernel of every bottleneck's first convolution (1: YOLOv5's C3; 3: YOLO11's C3k, whose bottlenecks are 3x3, 3x3)
    bool c3(int c1, int c2, int n, bool shortcut, const View *src, const View *low, const View *skip, View dst, int h, int w, const char *what,
            int k1 = 1)
    {
        const int c = c2 / 2;
        const long m = (long)p->B * h * w;
        const rva_conv_weights *cv[2] = {take(c1, c, 1, 1, what), take(c1, c, 1, 1, what)};
        const rva_conv_weights *cv3 = take(2 * c, c2, 1, 1, what);
        if (!cv[0] || !cv[1] || !cv3 || n < 1) return n < 1 ? fail("a C3 block needs at least one bottleneck") : false;
        View cat = buf(m, 3 * c);
        if (!cat.base) return false;
        if (low) { if (!upcat(cv, 2, *low, *skip, cat.sub(0, 2 * c), h, w)) return false; }
        else if (!conv(cv, 2, *src, cat.sub(0, 2 * c), h, w, 1)) return false;
        View x = cat.sub(0, c);
        for (int i = 0; i < n; ++i) {
            const rva_conv_weights *b1 = take(c, c, k1, 1, what), *b2 = take(c, c, 3, 1, what);
            // intermediate and output of every bottleneck in buffers of their own: with row windows a step rewrites part of its
            // output only, and the rest must still be what THIS bottleneck left there (see c2f)
            View tmp = buf(m, c), y = i == n - 1 ? cat.sub(2 * c, c) : buf(m, c);
            if (!tmp.base || !y.base) return false;
            if (!conv1(b1, x, tmp, h, w, 1) || !conv1(b2, tmp, y, h, w, 1, shortcut ? &x : nullptr)) return false;
            x = y;
        }
        if (!cv3->weight) return fail("convolution without weights");
        std::vector<float> &sw = pad_store.emplace_back((size_t)c2 * 2 * c, 0.f);
        for (int oc = 0; oc < c2; ++oc)
            for (int ic = 0; ic < 2 * c; ++ic) sw[(size_t)oc * 2 * c + ic] = cv3->weight[(size_t)oc * 2 * c + (ic + c) % (2 * c)];
        rva_conv_weights q = *cv3;
        q.weight = sw.data();
        return conv1(&pad_convs.emplace_back(q), cat.sub(c, 2 * c), dst, h, w, 1);
    }

    // fp16 stem from the planar input K1 writes, and the 3x3 s2 behind it: x1 = b1(b0(input)).  Stem weights [64][32] fp16, column
    // order k = 2 j + kx (kx in {0, 1}), k = 18 + j (kx = 2), j = c*3 + ky
    bool stem_f16(const rva_conv_weights *b0, const rva_conv_weights *b1, View *x1)
    {
        const rva_yolov8_desc &d = p->d;
        const int B = d.batch, H = d.height, W = d.width, c1 = d.widths[0], c2 = d.widths[1];
        const int h1 = H / 2, w1 = W / 2, h2 = H / 4, w2 = W / 4;
        if (c1 > 64) return fail("stem wider than 64 channels");
        if (!b0->weight) return fail("b0: no stem convolution");
        std::vector<_Float16> sw(64 * 32, (_Float16)0.f);
        std::vector<float> sb(64, 0.f);
        for (int co = 0; co < c1; ++co) {
            for (int j = 0; j < 9; ++j)                       // j = c*3 + ky;  weight[co][c][ky][kx]
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = b0->weight[((size_t)co * 3 + j / 3) * 9 + (j % 3) * 3 + kx];
                    sw[co * 32 + (kx < 2 ? 2 * j + kx : 18 + j)] = (_Float16)v;
                }
            if (b0->bias) sb[co] = b0->bias[co];
        }
        void *dsw = dev_alloc(sw.size() * 2, false), *dsb = dev_alloc(sb.size() * 4, false);
        if (!dsw || !dsb) return false;
        if (hipMemcpy(dsw, sw.data(), sw.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dsb, sb.data(), sb.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return fail("stem upload failed");
        *x1 = buf((long)B * h2 * w2, c2);
        if (!x1->base) return false;
        p->fused_stem = c1 == 32 && c2 == 64 && !(d.flags & RVA_PLAN_NO_STEM2);
        if (p->fused_stem) {
            Step s{}; s.kind = K_STEM2; s.w = dsw; s.b = (const float *)dsb; s.out = x1->ptr(); s.ldo = x1->ld; s.H = H; s.W = W;
            int ci, co, k, st;
            if (!pack(&b1, 1, &s.w2, &s.b2, &ci, &co, &k, &st)) return false;
            push(s, nullptr);
            return true;
        }
        View x0 = buf((long)B * h1 * w1, c1);
        if (!x0.base) return false;
        Step s{}; s.kind = K_STEM; s.w = dsw; s.b = (const float *)dsb; s.out = x0.ptr(); s.ldo = x0.ld; s.H = H; s.W = W; s.Cout = c1;
        push(s, nullptr);
        return conv1(b1, x0, *x1, h1, w1, 1);
    }

    // SPPF: cv1, three chained 5x5 max pools into the slices of one concat buffer, cv2
    bool sppf(int c5, View src, View dst, int h5, int w5)
    {
        const int c_ = c5 / 2;
        const rva_conv_weights *cv1 = take(c5, c_, 1, 1, "b9.cv1"), *cv2 = take(4 * c_, c5, 1, 1, "b9.cv2");
        View cat = buf((long)p->B * h5 * w5, 4 * c_);
        if (!cat.base || !conv1(cv1, src, cat.sub(0, c_), h5, w5, 1)) return false;
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
        return conv1(cv2, cat, dst, h5, w5, 1);
    }

    // Depthwise 3x3 (rva_dwconv3x3_nhwc_f16) over channels [c_off, c_off + dst.ch) of `c` (weight [C][1][3][3]): weights repacked
    // [9][dst.ch] fp16 (tap major).  Untunable; always the whole map.
    bool dwconv(const rva_conv_weights *c, int c_off, View src, View dst, int h, int w, int act, const View *res = nullptr)
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
        const void *db = nullptr;
        if (!upload(hw.data(), hw.size() * 2, &s.w) || !upload(hb.data(), hb.size() * 4, &db)) return false;
        s.b = (const float *)db;
        s.in = src.ptr(); s.ldi = src.ld; s.out = dst.ptr(); s.ldo = dst.ld; s.H = h; s.W = w; s.Cin = s.Cout = C; s.k = 3; s.stride = 1; s.act = act;
        if (res) { s.res = res->ptr(); s.ldr = res->ld; }
        push(s, nullptr);
        return true;
    }

    // YOLO11's C3k2: a C2f with c = c2 / 4 (quarter) or c2 / 2 whose inner blocks are bottlenecks 3x3 c -> c/2, 3x3 c/2 -> c, or
    // with c3k a C3 at width c / 2 with two 3x3, 3x3 bottlenecks, which writes its cv3 into the outer concat slice.  src as for c2f.
    bool c3k2(int c1, int c2, int n, bool c3k, bool quarter, bool shortcut, const View *src, const View *low, const View *skip, View dst, int h, int w,
              const char *what)
    {
        const int c = quarter ? c2 / 4 : c2 / 2;
        const long m = (long)p->B * h * w;
        if (n < 1 || c % 16) return fail("a C3k2 block needs at least one inner block and an inner width that is a multiple of 16");
        const rva_conv_weights *cv1 = take(c1, 2 * c, 1, 1, what), *cv2 = take((2 + n) * c, c2, 1, 1, what);
        if (!cv1 || !cv2) return false;
        View cat = buf(m, (2 + n) * c);
        if (!cat.base) return false;
        if (low) { if (!upcat(cv1, *low, *skip, cat.sub(0, 2 * c), h, w)) return false; }
        else if (!conv1(cv1, *src, cat.sub(0, 2 * c), h, w, 1)) return false;
        for (int i = 0; i < n; ++i) {
            View x = cat.sub((1 + i) * c, c), y = cat.sub((2 + i) * c, c);
            if (c3k) {
                if (!c3(c, c, 2, shortcut, &x, nullptr, nullptr, y, h, w, what, 3)) return false;
                continue;
            }
            const rva_conv_weights *b1 = take(c, c / 2, 3, 1, what), *b2 = take(c / 2, c, 3, 1, what);
            View tmp = buf(m, c / 2);                       // one per bottleneck, as in c2f
            if (!tmp.base || !conv1(b1, x, tmp, h, w, 1) || !conv1(b2, tmp, y, h, w, 1, shortcut ? &x : nullptr)) return false;
        }
        return conv1(cv2, cat, dst, h, w, 1);
    }

    // YOLO11's C2PSA.  Every buffer slice has ONE writer (a windowed convolution rewrites part of its output only, see c2f), so
    // cv1 runs as two launches: `a` goes straight into cv2's input buffer, `b` into a buffer of its own, and the last block's
    // ffn writes the other half of cv2's input.  Attention and the positional encoding always run the whole map.
    bool c2psa(int c1, int n, int heads, View src, View dst, int h, int w)
    {
        const int c = c1 / 2;
        const long m = (long)p->B * h * w;
        if (n < 1 || heads * 64 != c) return fail("C2PSA: psa_heads * 64 must be half the width of the block, and psa_blocks >= 1");
        const rva_conv_weights *cv1 = take(c1, 2 * c, 1, 1, "10.cv1"), *cv2 = take(2 * c, c1, 1, 1, "10.cv2");
        if (!cv1 || !cv2) return false;
        if (!cv1->weight) return fail("convolution without weights");
        rva_conv_weights qa = *cv1, qb = *cv1;
        qa.cout = qb.cout = c;
        qb.weight = cv1->weight + (size_t)c * c1;
        if (cv1->bias) qb.bias = cv1->bias + c;
        View cat = buf(m, 2 * c), x = buf(m, c);
        if (!cat.base || !x.base) return false;
        if (!conv1(&pad_convs.emplace_back(qa), src, cat.sub(0, c), h, w, 1) || !conv1(&pad_convs.emplace_back(qb), src, x, h, w, 1)) return false;
        for (int i = 0; i < n; ++i) {
            const rva_conv_weights *qkv = take(c, 2 * c, 1, 1, "10.attn.qkv"), *proj = take(c, c, 1, 1, "10.attn.proj"), *pe = take(1, c, 3, 1, "10.attn.pe"),
                                   *f0 = take(c, 2 * c, 1, 1, "10.ffn.0"), *f1 = take(2 * c, c, 1, 1, "10.ffn.1");
            if (!qkv || !proj || !pe || !f0 || !f1) return false;
            View q = buf(m, 2 * c), ao = buf(m, c), xo = buf(m, c), x1 = buf(m, c), f = buf(m, 2 * c);
            View y = i == n - 1 ? cat.sub(c, c) : buf(m, c);
            if (!q.base || !ao.base || !xo.base || !x1.base || !f.base || !y.base) return false;
            if (!conv1(qkv, x, q, h, w, 0)) return false;
            Step s{}; s.kind = K_ATTN; s.in = q.ptr(); s.ldi = q.ld; s.out = ao.ptr(); s.ldo = ao.ld; s.H = h; s.W = w; s.Cin = 2 * c; s.Cout = c; s.mode = heads;
            push(s, nullptr);
            for (int hd = 0; hd < heads; ++hd) {            // a head's v slice is contiguous, the heads' are not: one launch per head
                const View r = ao.sub(64 * hd, 64);
                if (!dwconv(pe, 64 * hd, q.sub(128 * hd + 64, 64), xo.sub(64 * hd, 64), h, w, 0, &r)) return false;
            }
            if (!conv1(proj, xo, x1, h, w, 0, &x)) return false;
            if (!conv1(f0, x1, f, h, w, 1) || !conv1(f1, f, y, h, w, 0, &x1)) return false;
            x = y;
        }
        return conv1(cv2, cat, dst, h, w, 1);
    }

    bool build_11(const rva_yolo11_desc &e)
    {
        const rva_yolov8_desc &d = p->d;
        const int B = d.batch, H = d.height, W = d.width;
        const int c1 = d.widths[0], c2 = d.widths[1], c3w = d.widths[2], c4 = d.widths[3], c5 = d.widths[4];
        const int h2 = H / 4, w2 = W / 4, h3 = H / 8, w3 = W / 8, h4 = H / 16, w4 = W / 16, h5 = H / 32, w5 = W / 32;
        const rva_conv_weights *b0 = take(3, c1, 3, 2, "0"), *b1 = take(c1, c2, 3, 2, "1");
        View x1;
        if (!b0 || !b1 || !stem_f16(b0, b1, &x1)) return false;
        auto block = [&](int i, int ci, int co, bool quarter, bool shortcut, const View *src, const View *low, const View *skip, View dst, int h, int w,
                         const char *what) {
            return c3k2(ci, co, e.repeats[i], e.c3k[i] != 0, quarter, shortcut, src, low, skip, dst, h, w, what);
        };
        // concat buffers of the neck: producers write their slice directly.  cat13 = [up(p5) | p4], cat16 = [up(n4) | p3],
        // cat19 = [17 | n4], cat22 = [20 | p5]
        View cat13 = buf((long)B * h4 * w4, c5 + c4), cat16 = buf((long)B * h3 * w3, c4 + c4), cat19 = buf((long)B * h4 * w4, c3w + c4),
             cat22 = buf((long)B * h5 * w5, c4 + c5);
        if (!cat13.base || !cat16.base || !cat19.base || !cat22.base) return false;
        View p4 = cat13.sub(c5, c4), p3 = cat16.sub(c4, c4), n4 = cat19.sub(c3w, c4), p5 = cat22.sub(c4, c5);
        View x2 = buf((long)B * h2 * w2, c3w), t3 = buf((long)B * h3 * w3, c3w), t4 = buf((long)B * h4 * w4, c4);
        if (!x2.base || !t3.base || !t4.base) return false;
        if (!block(0, c2, c3w, true, true, &x1, nullptr, nullptr, x2, h2, w2, "2")) return false;
        if (!conv1(take(c3w, c3w, 3, 2, "3"), x2, t3, h2, w2, 1)) return false;
        if (!block(1, c3w, c4, true, true, &t3, nullptr, nullptr, p3, h3, w3, "4")) return false;
        if (!conv1(take(c4, c4, 3, 2, "5"), p3, t4, h3, w3, 1)) return false;
        if (!block(2, c4, c4, false, true, &t4, nullptr, nullptr, p4, h4, w4, "6")) return false;
        View t5 = buf((long)B * h5 * w5, c5), t5b = buf((long)B * h5 * w5, c5), t5c = buf((long)B * h5 * w5, c5);
        p->quiet_step = (int)p->steps.size();
        if (!t5.base || !t5b.base || !t5c.base || !conv1(take(c4, c5, 3, 2, "7"), p4, t5, h4, w4, 1)) return false;
        if (!block(3, c5, c5, false, true, &t5, nullptr, nullptr, t5b, h5, w5, "8")) return false;
        if (!sppf(c5, t5b, t5c, h5, w5)) return false;
        if (!c2psa(c5, e.psa_blocks, e.psa_heads, t5c, p5, h5, w5)) return false;
        View n3 = buf((long)B * h3 * w3, c3w);
        if (!n3.base) return false;
        if (c5 % 64 == 0 && c4 % 64 == 0 && h4 == 2 * h5 && w4 == 2 * w5 && h3 == 2 * h4 && w3 == 2 * w4) {
            // FPN top-down path: upsample + concat folded into the consuming 1x1 convolutions (rva_conv1x1_upcat_f16)
            if (!block(4, c5 + c4, c4, false, false, nullptr, &p5, &p4, n4, h4, w4, "13")) return false;
            if (!block(5, c4 + c4, c3w, false, false, nullptr, &n4, &p3, n3, h3, w3, "16")) return false;
        } else {
            Step u1{}; u1.kind = K_UP2; u1.in = p5.ptr(); u1.ldi = p5.ld; u1.out = cat13.sub(0, c5).ptr(); u1.ldo = cat13.ld; u1.H = h5; u1.W = w5; u1.Cin = c5;
            push(u1, nullptr);
            if (!block(4, c5 + c4, c4, false, false, &cat13, nullptr, nullptr, n4, h4, w4, "13")) return false;
            Step u2{}; u2.kind = K_UP2; u2.in = n4.ptr(); u2.ldi = n4.ld; u2.out = cat16.sub(0, c4).ptr(); u2.ldo = cat16.ld; u2.H = h4; u2.W = w4; u2.Cin = c4;
            push(u2, nullptr);
            if (!block(5, c4 + c4, c3w, false, false, &cat16, nullptr, nullptr, n3, h3, w3, "16")) return false;
        }
        if (!conv1(take(c3w, c3w, 3, 2, "17"), n3, cat19.sub(0, c3w), h3, w3, 1)) return false;
        View m4 = buf((long)B * h4 * w4, c4), m5 = buf((long)B * h5 * w5, c5);
        if (!m4.base || !m5.base) return false;
        if (!block(6, c3w + c4, c4, false, false, &cat19, nullptr, nullptr, m4, h4, w4, "19")) return false;
        if (!conv1(take(c4, c4, 3, 2, "20"), m4, cat22.sub(0, c4), h4, w4, 1)) return false;
        if (!block(7, c4 + c5, c5, false, false, &cat22, nullptr, nullptr, m5, h5, w5, "22")) return false;
        // detect head: the box branch is YOLOv8's; the class branch is dw3x3, 1x1, dw3x3, 1x1, 1x1 with its interior width rounded
        // up to 8 (zero-extended weights: a pad channel is SiLU(0) = 0 through the depthwise steps and meets zero weights)
        int cb = c3w / 4 > 64 ? c3w / 4 : 64;
        const int ncm = d.nc < 100 ? d.nc : 100, cc_real = c3w > ncm ? c3w : ncm;
        const int cc = (cc_real + 7) / 8 * 8, ncp = (d.nc + 7) / 8 * 8;
        p->A = h3 * w3 + h4 * w4 + h5 * w5;
        const rva_conv_weights *box[3][3], *cls[3][5];
        const int chs[3] = {c3w, c4, c5};
        for (int l = 0; l < 3; ++l) {
            box[l][0] = take(chs[l], cb, 3, 1, "detect.box.0"); box[l][1] = take(cb, cb, 3, 1, "detect.box.1"); box[l][2] = take(cb, 64, 1, 1, "detect.box.2");
            if (!box[l][0] || !box[l][1] || !box[l][2]) return false;
        }
        for (int l = 0; l < 3; ++l) {
            cls[l][0] = take(1, chs[l], 3, 1, "detect.cls.0.0"); cls[l][1] = take(chs[l], cc_real, 1, 1, "detect.cls.0.1");
            cls[l][2] = take(1, cc_real, 3, 1, "detect.cls.1.0"); cls[l][3] = take(cc_real, cc_real, 1, 1, "detect.cls.1.1");
            cls[l][4] = take(cc_real, d.nc, 1, 1, "detect.cls.2");
            for (int i = 0; i < 5; ++i)
                if (!cls[l][i]) return false;
            cls[l][1] = padded(cls[l][1], chs[l], cc); cls[l][2] = padded(cls[l][2], 1, cc); cls[l][3] = padded(cls[l][3], cc, cc);
            cls[l][4] = padded(cls[l][4], cc, ncp);
        }
        if (next != d.n_convs) return fail("convolution list longer than the architecture");
        p->fused_head = cb % 64 == 0 && cc % 64 == 0;
        const View feats[3] = {n3, m4, m5};
        const int hs[3] = {h3, h4, h5}, ws[3] = {w3, w4, w5};
        const float strides[3] = {8.f, 16.f, 32.f};
        Step h3s{}; h3s.kind = K_HEAD3;
        int a0 = 0;
        for (int l = 0; l < 3; ++l) {
            const long m = (long)B * hs[l] * ws[l];
            View bb1 = buf(m, cb), bb2 = buf(m, cb), d1 = buf(m, chs[l]), k1 = buf(m, cc), d2 = buf(m, cc), k2 = buf(m, cc);
            if (!bb1.base || !bb2.base || !d1.base || !k1.base || !d2.base || !k2.base) return false;
            if (!conv1(box[l][0], feats[l], bb1, hs[l], ws[l], 1) || !conv1(box[l][1], bb1, bb2, hs[l], ws[l], 1)) return false;
            if (!dwconv(cls[l][0], 0, feats[l], d1, hs[l], ws[l], 1) || !conv1(cls[l][1], d1, k1, hs[l], ws[l], 1) ||
                !dwconv(cls[l][2], 0, k1, d2, hs[l], ws[l], 1) || !conv1(cls[l][3], d2, k2, hs[l], ws[l], 1)) return false;
            if (p->fused_head) {
                if (!head(box[l][2], bb2, 1, hs[l], ws[l], a0, strides[l]) || !head(cls[l][4], k2, 2, hs[l], ws[l], a0, strides[l])) return false;
            } else {
                View bo = buf(m, 64), ko = buf(m, ncp);
                if (!bo.base || !ko.base) return false;
                if (!conv1(box[l][2], bb2, bo, hs[l], ws[l], 0) || !conv1(cls[l][4], k2, ko, hs[l], ws[l], 0)) return false;
                h3s.hb[l] = bo.ptr(); h3s.hldb[l] = bo.ld; h3s.hk[l] = ko.ptr(); h3s.hldc[l] = ko.ld; h3s.hh[l] = hs[l]; h3s.hw[l] = ws[l]; h3s.hs[l] = strides[l];
            }
            a0 += hs[l] * ws[l];
        }
        if (!p->fused_head) push(h3s, nullptr);
        return err.empty();
    }

    bool build_v5(const float *anchors)
    {
        const rva_yolov8_desc &d = p->d;
        const int B = d.batch, H = d.height, W = d.width;
        const int c1 = d.widths[0], c2 = d.widths[1], c3w = d.widths[2], c4 = d.widths[3], c5 = d.widths[4];
        const int h1 = H / 2, w1 = W / 2, h2 = H / 4, w2 = W / 4, h3 = H / 8, w3 = W / 8, h4 = H / 16, w4 = W / 16, h5 = H / 32, w5 = W / 32;
        const int nh = d.depth_head;
        if (c1 > 64) return fail("stem wider than 64 channels");
        if (c3w % 64 || c4 % 64 || c5 % 64) return fail("YOLOv5 plan: c3, c4 and c5 must be multiples of 64 (the upsample + concat and head kernels)");
        const rva_conv_weights *b0 = take(3, c1, 6, 2, "b0");
        if (!b0 || !b0->weight) return fail("b0: no stem convolution");
        {   // stem (planar input from K1): weights [64][128] fp16 in the checkpoint's own (c, ky, kx) order, zero-padded
            std::vector<_Float16> sw(64 * 128, (_Float16)0.f);
            std::vector<float> sb(64, 0.f);
            for (int co = 0; co < c1; ++co) {
                for (int k = 0; k < 108; ++k) sw[co * 128 + k] = (_Float16)b0->weight[(size_t)co * 108 + k];
                if (b0->bias) sb[co] = b0->bias[co];
            }
            Step s{}; s.kind = K_STEM6;
            const void *db = nullptr;
            if (!upload(sw.data(), sw.size() * 2, &s.w) || !upload(sb.data(), sb.size() * 4, &db)) return false;
            s.b = (const float *)db;
            View x0 = buf((long)B * h1 * w1, c1);
            if (!x0.base) return false;
            s.out = x0.ptr(); s.ldo = x0.ld; s.H = H; s.W = W; s.Cout = c1;
            push(s, nullptr);
            View x1 = buf((long)B * h2 * w2, c2), x2 = buf((long)B * h2 * w2, c2);
            if (!x1.base || !x2.base || !conv1(take(c1, c2, 3, 2, "b1"), x0, x1, h1, w1, 1)) return false;
            if (!c3(c2, c2, d.depth_backbone[0], true, &x1, nullptr, nullptr, x2, h2, w2, "b2")) return false;
            View t3 = buf((long)B * h3 * w3, c3w), p3 = buf((long)B * h3 * w3, c3w);
            if (!t3.base || !p3.base || !conv1(take(c2, c3w, 3, 2, "b3"), x2, t3, h2, w2, 1)) return false;
            if (!c3(c3w, c3w, d.depth_backbone[1], true, &t3, nullptr, nullptr, p3, h3, w3, "b4")) return false;
            View t4 = buf((long)B * h4 * w4, c4), p4 = buf((long)B * h4 * w4, c4);
            if (!t4.base || !p4.base || !conv1(take(c3w, c4, 3, 2, "b5"), p3, t4, h3, w3, 1)) return false;
            if (!c3(c4, c4, d.depth_backbone[2], true, &t4, nullptr, nullptr, p4, h4, w4, "b6")) return false;
            View t5 = buf((long)B * h5 * w5, c5), t5b = buf((long)B * h5 * w5, c5), p5 = buf((long)B * h5 * w5, c5);
            p->quiet_step = (int)p->steps.size();
            if (!t5.base || !t5b.base || !p5.base || !conv1(take(c4, c5, 3, 2, "b7"), p4, t5, h4, w4, 1)) return false;
            if (!c3(c5, c5, d.depth_backbone[3], true, &t5, nullptr, nullptr, t5b, h5, w5, "b8")) return false;
            if (!sppf(c5, t5b, p5, h5, w5)) return false;
            // neck: the two concat buffers of the bottom-up path; h10 / h14 write their slices directly
            View cat20 = buf((long)B * h4 * w4, 2 * c3w), cat23 = buf((long)B * h5 * w5, 2 * c4);
            if (!cat20.base || !cat23.base) return false;
            View t10 = cat23.sub(c4, c4), t14 = cat20.sub(c3w, c3w);
            View n4 = buf((long)B * h4 * w4, c4), n3 = buf((long)B * h3 * w3, c3w), m4 = buf((long)B * h4 * w4, c4), m5 = buf((long)B * h5 * w5, c5);
            if (!n4.base || !n3.base || !m4.base || !m5.base) return false;
            if (!conv1(take(c5, c4, 1, 1, "h10"), p5, t10, h5, w5, 1)) return false;
            if (!c3(2 * c4, c4, nh, false, nullptr, &t10, &p4, n4, h4, w4, "h13")) return false;
            if (!conv1(take(c4, c3w, 1, 1, "h14"), n4, t14, h4, w4, 1)) return false;
            if (!c3(2 * c3w, c3w, nh, false, nullptr, &t14, &p3, n3, h3, w3, "h17")) return false;
            if (!conv1(take(c3w, c3w, 3, 2, "h18"), n3, cat20.sub(0, c3w), h3, w3, 1)) return false;
            if (!c3(2 * c3w, c4, nh, false, &cat20, nullptr, nullptr, m4, h4, w4, "h20")) return false;
            if (!conv1(take(c4, c4, 3, 2, "h21"), m4, cat23.sub(0, c4), h4, w4, 1)) return false;
            if (!c3(2 * c4, c5, nh, false, &cat23, nullptr, nullptr, m5, h5, w5, "h23")) return false;
            // detect: one fused convolution + decode per level, into disjoint anchor ranges of the output
            const int no = 5 + d.nc, co_real = 3 * no, co = (co_real + 7) / 8 * 8;
            p->A = 3 * (h3 * w3 + h4 * w4 + h5 * w5);
            const View feats[3] = {n3, m4, m5};
            const int chs[3] = {c3w, c4, c5}, hs[3] = {h3, h4, h5}, ws[3] = {w3, w4, w5};
            const float strides[3] = {8.f, 16.f, 32.f};
            const void *danc = nullptr;
            if (!upload(anchors, sizeof(float) * 18, &danc)) return false;
            int a0 = 0;
            for (int l = 0; l < 3; ++l) {
                const rva_conv_weights *hc = padded(take(chs[l], co_real, 1, 1, "detect.m"), chs[l], co);
                if (!hc) return false;
                Step s{}; s.kind = K_HEAD5;
                if (!pack(&hc, 1, &s.w, &s.b, &s.Cin, &s.Cout, &s.k, &s.stride)) return false;
                s.in = feats[l].ptr(); s.ldi = feats[l].ld; s.H = hs[l]; s.W = ws[l]; s.a0 = a0; s.stride_px = strides[l];
                s.b2 = (const float *)danc + 6 * l;
                push(s, "head5:%d->%d k1s1 %dx%d", s.Cin, s.Cout, hs[l], ws[l]);
                a0 += 3 * hs[l] * ws[l];
            }
            if (next != d.n_convs) return fail("convolution list longer than the architecture");
        }
        return err.empty();
    }

    bool build()
    {
        const rva_yolov8_desc &d = p->d;
        const int B = d.batch, H = d.height, W = d.width;
        const int c1 = d.widths[0], c2 = d.widths[1], c3 = d.widths[2], c4 = d.widths[3], c5 = d.widths[4];
        const int h1 = H / 2, w1 = W / 2, h2 = H / 4, w2 = W / 4, h3 = H / 8, w3 = W / 8, h4 = H / 16, w4 = W / 16, h5 = H / 32, w5 = W / 32;
        const int nh = d.depth_head;
        // stem (planar input from K1): weights [64][32] fp16, column order k = 2 j + kx (kx in {0, 1}), k = 18 + j (kx = 2), j = c*3 + ky
        const rva_conv_weights *b0 = take(3, c1, 3, 2, "b0"), *b1 = take(c1, c2, 3, 2, "b1");
        if (!b0 || !b1) return false;
        View x1;
        if (p->f32) {
            // stem from the planar fp32 input (rva_stem_conv_f32): the checkpoint's [c1][3][3][3] weights as they are
            Step s{}; s.kind = K_STEM_F32;
            std::vector<float> sb(c1, 0.f);
            if (b0->bias) memcpy(sb.data(), b0->bias, sizeof(float) * c1);
            const void *db = nullptr;
            if (!b0->weight || !upload(b0->weight, sizeof(float) * c1 * 27, &s.w) || !upload(sb.data(), sizeof(float) * c1, &db)) return false;
            s.b = (const float *)db;
            View x0 = buf((long)B * h1 * w1, c1);
            x1 = buf((long)B * h2 * w2, c2);
            if (!x0.base || !x1.base) return false;
            s.out = x0.ptr(); s.ldo = x0.ld; s.H = H; s.W = W; s.Cout = c1;
            push(s, nullptr);
            if (!conv1(b1, x0, x1, h1, w1, 1)) return false;
        } else if (!stem_f16(b0, b1, &x1)) return false;
        View x2 = buf((long)B * h2 * w2, c2);
        if (!x2.base || !c2f(c2, c2, d.depth_backbone[0], true, &x1, nullptr, nullptr, x2, h2, w2, "b2")) return false;
        // concat buffers of the neck: producers write their slice directly
        View cat15 = buf((long)B * h3 * w3, c4 + c3), cat12 = buf((long)B * h4 * w4, c5 + c4), cat18 = buf((long)B * h4 * w4, c3 + c4),
             cat21 = buf((long)B * h5 * w5, c4 + c5);
        if (!cat15.base || !cat12.base || !cat18.base || !cat21.base) return false;
        View p3 = cat15.sub(c4, c3), p4 = cat12.sub(c5, c4), n4 = cat18.sub(c3, c4), p5 = cat21.sub(c4, c5);
        View t3 = buf((long)B * h3 * w3, c3);
        if (!t3.base || !conv1(take(c2, c3, 3, 2, "b3"), x2, t3, h2, w2, 1)) return false;
        if (!c2f(c3, c3, d.depth_backbone[1], true, &t3, nullptr, nullptr, p3, h3, w3, "b4")) return false;
        View t4 = buf((long)B * h4 * w4, c4);
        if (!t4.base || !conv1(take(c3, c4, 3, 2, "b5"), p3, t4, h3, w3, 1)) return false;
        if (!c2f(c4, c4, d.depth_backbone[2], true, &t4, nullptr, nullptr, p4, h4, w4, "b6")) return false;
        View t5 = buf((long)B * h5 * w5, c5);
        p->quiet_step = (int)p->steps.size();
        if (!t5.base || !conv1(take(c4, c5, 3, 2, "b7"), p4, t5, h4, w4, 1)) return false;
        View t5b = buf((long)B * h5 * w5, c5);
        if (!t5b.base || !c2f(c5, c5, d.depth_backbone[3], true, &t5, nullptr, nullptr, t5b, h5, w5, "b8")) return false;
        if (!sppf(c5, t5b, p5, h5, w5)) return false;
        const bool fuse_up = !p->f32 && c5 % 64 == 0 && c4 % 64 == 0 && c3 % 64 == 0 && h4 == 2 * h5 && w4 == 2 * w5 && h3 == 2 * h4 && w3 == 2 * w4;
        View n3 = buf((long)B * h3 * w3, c3);
        if (!n3.base) return false;
        if (fuse_up) {    // FPN top-down path: upsample + concat folded into the consuming 1x1 convolutions
            if (!c2f(c5 + c4, c4, nh, false, nullptr, &p5, &p4, n4, h4, w4, "h12")) return false;
            if (!c2f(c4 + c3, c3, nh, false, nullptr, &n4, &p3, n3, h3, w3, "h15")) return false;
        } else {
            Step u1{}; u1.kind = p->f32 ? K_UP2_F32 : K_UP2; u1.in = p5.ptr(); u1.ldi = p5.ld; u1.out = cat12.sub(0, c5).ptr(); u1.ldo = cat12.ld; u1.H = h5; u1.W = w5; u1.Cin = c5;
            push(u1, nullptr);
            if (!c2f(c5 + c4, c4, nh, false, &cat12, nullptr, nullptr, n4, h4, w4, "h12")) return false;
            Step u2{}; u2.kind = p->f32 ? K_UP2_F32 : K_UP2; u2.in = n4.ptr(); u2.ldi = n4.ld; u2.out = cat15.sub(0, c4).ptr(); u2.ldo = cat15.ld; u2.H = h4; u2.W = w4; u2.Cin = c4;
            push(u2, nullptr);
            if (!c2f(c4 + c3, c3, nh, false, &cat15, nullptr, nullptr, n3, h3, w3, "h15")) return false;
        }
        const int fork_n3 = (int)p->steps.size();            // n3 is complete here: the stride-8 detect branch may start
        if (!conv1(take(c3, c3, 3, 2, "h16"), n3, cat18.sub(0, c3), h3, w3, 1)) return false;
        View m4 = buf((long)B * h4 * w4, c4);
        if (!m4.base || !c2f(c3 + c4, c4, nh, false, &cat18, nullptr, nullptr, m4, h4, w4, "h18")) return false;
        const int fork_m4 = (int)p->steps.size();            // m4 is complete: the stride-16 detect branch may start
        if (!conv1(take(c4, c4, 3, 2, "h19"), m4, cat21.sub(0, c4), h4, w4, 1)) return false;
        View m5 = buf((long)B * h5 * w5, c5);
        if (!m5.base || !c2f(c4 + c5, c5, nh, false, &cat21, nullptr, nullptr, m5, h5, w5, "h21")) return false;
        // detect head
        const int rm4 = 4 * d.reg_max;
        int cb = c3 / 4 > rm4 ? c3 / 4 : rm4;
        if (cb < 16) cb = 16;
        const int cc_real = c3 > (d.nc < 100 ? d.nc : 100) ? c3 : (d.nc < 100 ? d.nc : 100);
        // what the class branch runs with: interior width a multiple of 8 (16 where an fp32 convolution reads it), ncp logit columns
        const int cal = p->f32 ? 16 : 8;
        const int cc = (cc_real + cal - 1) / cal * cal, ncp = (d.nc + 7) / 8 * 8;
        p->A = h3 * w3 + h4 * w4 + h5 * w5;
        // module order: all box branches first, then all class branches
        const rva_conv_weights *box[3][3], *cls[3][3];
        const int chs[3] = {c3, c4, c5};
        for (int l = 0; l < 3; ++l) {
            box[l][0] = take(chs[l], cb, 3, 1, "detect.box.0"); box[l][1] = take(cb, cb, 3, 1, "detect.box.1"); box[l][2] = take(cb, rm4, 1, 1, "detect.box.2");
            if (!box[l][0] || !box[l][1] || !box[l][2]) return false;
        }
        for (int l = 0; l < 3; ++l) {
            cls[l][0] = take(chs[l], cc_real, 3, 1, "detect.cls.0"); cls[l][1] = take(cc_real, cc_real, 3, 1, "detect.cls.1");
            cls[l][2] = take(cc_real, d.nc, 1, 1, "detect.cls.2");
            if (!cls[l][0] || !cls[l][1] || !cls[l][2]) return false;
            cls[l][0] = padded(cls[l][0], chs[l], cc); cls[l][1] = padded(cls[l][1], cc, cc); cls[l][2] = padded(cls[l][2], cc, ncp);
        }
        if (next != d.n_convs) return fail("convolution list longer than the architecture");
        p->fused_head = !p->f32 && cb % 64 == 0 && cc % 64 == 0 && rm4 == 64;
        const View feats[3] = {n3, m4, m5};
        const int hs[3] = {h3, h4, h5}, ws[3] = {w3, w4, w5};
        const float strides[3] = {8.f, 16.f, 32.f};
        Step h3s{}; h3s.kind = K_HEAD3;
        int a0 = 0;
        for (int l = 0; l < 3; ++l) {
            // the three detect branches only depend on their own feature map and write disjoint anchor ranges: the stride-8 and
            // stride-16 branches may run on side streams beside the rest of the neck (rva_yolov8_plan_run_lanes)
            lane = ((p->fused_head || p->f32) && l < 2) ? l + 1 : 0;
            if (lane) p->fork_step[lane] = l == 0 ? fork_n3 : fork_m4;
            const long m = (long)B * hs[l] * ws[l];
            View first = buf(m, cb + cc), b2 = buf(m, cb), k2 = buf(m, cc);
            if (!first.base || !b2.base || !k2.base) return false;
            const rva_conv_weights *sib[2] = {box[l][0], cls[l][0]};
            if (!conv(sib, 2, feats[l], first, hs[l], ws[l], 1)) return false;      // one launch, Cout = cb + cc
            if (p->fused_head) {
                if (!conv1(box[l][1], first.sub(0, cb), b2, hs[l], ws[l], 1) || !head(box[l][2], b2, 1, hs[l], ws[l], a0, strides[l])) return false;
                if (!conv1(cls[l][1], first.sub(cb, cc), k2, hs[l], ws[l], 1) || !head(cls[l][2], k2, 2, hs[l], ws[l], a0, strides[l])) return false;
            } else {
                View bo = buf(m, rm4), ko = buf(m, ncp);
                if (!bo.base || !ko.base) return false;
                if (!conv1(box[l][1], first.sub(0, cb), b2, hs[l], ws[l], 1) || !conv1(box[l][2], b2, bo, hs[l], ws[l], 0)) return false;
                if (!conv1(cls[l][1], first.sub(cb, cc), k2, hs[l], ws[l], 1) || !conv1(cls[l][2], k2, ko, hs[l], ws[l], 0)) return false;
                h3s.hb[l] = bo.ptr(); h3s.hldb[l] = bo.ld; h3s.hk[l] = ko.ptr(); h3s.hldc[l] = ko.ld; h3s.hh[l] = hs[l]; h3s.hw[l] = ws[l]; h3s.hs[l] = strides[l];
                if (p->f32) {             // the level's decode on its own lane (rva_yolo_head_f32): disjoint anchor range of the output
                    Step hs1{}; hs1.kind = K_HEAD_F32; hs1.in = bo.ptr(); hs1.ldi = bo.ld; hs1.in2 = ko.ptr(); hs1.ldi2 = ko.ld;
                    hs1.H = hs[l]; hs1.W = ws[l]; hs1.a0 = a0; hs1.stride_px = strides[l];
                    push(hs1, nullptr);
                }
            }
            a0 += hs[l] * ws[l];
        }
        lane = 0;
        if (!p->fused_head && !p->f32) push(h3s, nullptr);
        return err.empty();
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

}  // namespace

extern "C" {

int rva_yolov8_plan_create(rva_ctx *ctx, const rva_yolov8_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out)
{
    if (!ctx || !desc || !convs || !out) return RVA_ERR_ARG;
    *out = nullptr;
    if (desc->batch <= 0 || desc->height <= 0 || desc->width <= 0 || desc->height % 32 || desc->width % 32 || desc->nc < 1 ||
        desc->nc > 1024 || desc->reg_max != 16 || desc->n_convs <= 0)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolov8_plan_create: batch > 0, height and width multiples of 32, 1 <= nc <= 1024, reg_max 16");
    for (int i = 0; i < 5; ++i)
        if (desc->widths[i] <= 0 || desc->widths[i] % 8) return rva_fail(ctx, RVA_ERR_ARG, "rva_yolov8_plan_create: channel widths must be multiples of 8");
    RVA_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<rva_yolov8_plan> p(new rva_yolov8_plan());
    p->ctx = ctx; p->d = *desc; p->B = desc->batch; p->H = desc->height; p->W = desc->width; p->nc = desc->nc;
    p->head_rows = 4 + desc->nc;
    p->f32 = (desc->flags & RVA_PLAN_F32) != 0;
    p->box32 = (desc->flags & RVA_PLAN_BOX_F32) != 0;
    if (p->f32 && p->box32)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolov8_plan_create: RVA_PLAN_BOX_F32 belongs to fp16 plans (the output of an RVA_PLAN_F32 plan is fp32 already)");
    Builder b{p.get(), convs};
    const bool ok = b.build();
    if (!ok) {
        for (void *a : p->allocs) (void)hipFree(a);
        return rva_fail(ctx, b.err.find("hip") == 0 || b.err.find("upload") != std::string::npos ? RVA_ERR_HIP : RVA_ERR_ARG,
                        "rva_yolov8_plan_create: %s", b.err.c_str());
    }
    for (int l = 1; l <= 2; ++l)
        if (p->fork_step[l] >= 0) {
            RVA_HIP(ctx, hipEventCreateWithFlags(&p->fork_ev[l], hipEventDisableTiming));
            RVA_HIP(ctx, hipEventCreateWithFlags(&p->join_ev[l], hipEventDisableTiming));
        }
    RVA_HIP(ctx, hipDeviceSynchronize());                  // weights are in place before the first run on any stream
    if (p->box32) p->box_off = ((size_t)p->B * (4 + p->nc) * p->A * 2 + 255) / 256 * 256;
    p->rows_top = 0; p->rows_bottom = p->H;
    propagate_rows(p.get());
    *out = p.release();
    return RVA_OK;
}

int rva_yolov5_plan_create(rva_ctx *ctx, const rva_yolov5_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out)
{
    if (!ctx || !desc || !convs || !out) return RVA_ERR_ARG;
    *out = nullptr;
    if (desc->batch <= 0 || desc->height <= 0 || desc->width <= 0 || desc->height % 32 || desc->width % 32 || desc->nc < 1 ||
        desc->nc > 1024 || desc->n_convs <= 0)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolov5_plan_create: batch > 0, height and width multiples of 32, 1 <= nc <= 1024");
    if (desc->flags & RVA_PLAN_F32)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolov5_plan_create: there is no fp32 YOLOv5 plan (RVA_PLAN_F32); build the fp16 plan");
    for (int i = 0; i < 5; ++i)
        if (desc->widths[i] <= 0 || desc->widths[i] % 8) return rva_fail(ctx, RVA_ERR_ARG, "rva_yolov5_plan_create: channel widths must be multiples of 8");
    for (int i = 0; i < 18; ++i)
        if (!(desc->anchors[i] > 0.f) || !(desc->anchors[i] < 65504.f)) return rva_fail(ctx, RVA_ERR_ARG, "rva_yolov5_plan_create: anchors must be positive pixel sizes");
    RVA_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<rva_yolov8_plan> p(new rva_yolov8_plan());
    p->ctx = ctx; p->B = desc->batch; p->H = desc->height; p->W = desc->width; p->nc = desc->nc;
    p->d.batch = desc->batch; p->d.height = desc->height; p->d.width = desc->width; p->d.nc = desc->nc; p->d.reg_max = 0;
    for (int i = 0; i < 5; ++i) p->d.widths[i] = desc->widths[i];
    for (int i = 0; i < 4; ++i) p->d.depth_backbone[i] = desc->depth_backbone[i];
    p->d.depth_head = desc->depth_head; p->d.n_convs = desc->n_convs; p->d.flags = desc->flags;
    p->head_rows = 5 + desc->nc;
    p->box32 = (desc->flags & RVA_PLAN_BOX_F32) != 0;
    Builder b{p.get(), convs};
    if (!b.build_v5(desc->anchors)) {
        for (void *a : p->allocs) (void)hipFree(a);
        return rva_fail(ctx, b.err.find("hip") == 0 || b.err.find("upload") != std::string::npos ? RVA_ERR_HIP : RVA_ERR_ARG,
                        "rva_yolov5_plan_create: %s", b.err.c_str());
    }
    RVA_HIP(ctx, hipDeviceSynchronize());                  // weights are in place before the first run on any stream
    if (p->box32) p->box_off = ((size_t)p->B * p->head_rows * p->A * 2 + 255) / 256 * 256;
    p->rows_top = 0; p->rows_bottom = p->H;
    propagate_rows(p.get());
    *out = p.release();
    return RVA_OK;
}

int rva_yolo11_plan_create(rva_ctx *ctx, const rva_yolo11_desc *desc, const rva_conv_weights *convs, rva_yolov8_plan **out)
{
    if (!ctx || !desc || !convs || !out) return RVA_ERR_ARG;
    *out = nullptr;
    if (desc->batch <= 0 || desc->height <= 0 || desc->width <= 0 || desc->height % 32 || desc->width % 32 || desc->nc < 1 ||
        desc->nc > 1024 || desc->n_convs <= 0)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo11_plan_create: batch > 0, height and width multiples of 32, 1 <= nc <= 1024");
    if (desc->flags & RVA_PLAN_F32)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo11_plan_create: there is no fp32 YOLO11 plan (RVA_PLAN_F32); build the fp16 plan");
    for (int i = 0; i < 5; ++i)
        if (desc->widths[i] <= 0 || desc->widths[i] % 8) return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo11_plan_create: channel widths must be multiples of 8");
    if (desc->psa_heads < 1 || desc->psa_heads * 128 != desc->widths[4])
        return rva_fail(ctx, RVA_ERR_ARG, "rva_yolo11_plan_create: psa_heads * 64 = %d is not half the C2PSA width %d", desc->psa_heads * 64, desc->widths[4]);
    RVA_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<rva_yolov8_plan> p(new rva_yolov8_plan());
    p->ctx = ctx; p->B = desc->batch; p->H = desc->height; p->W = desc->width; p->nc = desc->nc;
    p->d.batch = desc->batch; p->d.height = desc->height; p->d.width = desc->width; p->d.nc = desc->nc; p->d.reg_max = 16;
    for (int i = 0; i < 5; ++i) p->d.widths[i] = desc->widths[i];
    p->d.n_convs = desc->n_convs; p->d.flags = desc->flags;
    p->head_rows = 4 + desc->nc;
    p->box32 = (desc->flags & RVA_PLAN_BOX_F32) != 0;
    Builder b{p.get(), convs};
    if (!b.build_11(*desc)) {
        for (void *a : p->allocs) (void)hipFree(a);
        return rva_fail(ctx, b.err.find("hip") == 0 || b.err.find("upload") != std::string::npos ? RVA_ERR_HIP : RVA_ERR_ARG,
                        "rva_yolo11_plan_create: %s", b.err.c_str());
    }
    RVA_HIP(ctx, hipDeviceSynchronize());                  // weights are in place before the first run on any stream
    if (p->box32) p->box_off = ((size_t)p->B * p->head_rows * p->A * 2 + 255) / 256 * 256;
    p->rows_top = 0; p->rows_bottom = p->H;
    propagate_rows(p.get());
    *out = p.release();
    return RVA_OK;
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
