// K8: baseline JPEG decoder on the device -- the "decode" half of SURVEY.md 8f-3 for Motion-JPEG sources.
//
// Stands where VideoStream.open() / frames() sit on cv2.VideoCapture(url) (video_stream.py:76,173) when the camera sends JPEG
// pictures: n compressed pictures in host memory go in, sizes and sampling mixed, and come out as frames in HBM, either libjpeg's
// own BGR picture (what cv2.imdecode and Pillow give, bit for bit) or an NV12 surface in the BT.601 limited range K1 assumes.
// The host half (rva_jpeg_parse.h) walks the markers into a descriptor per picture and finds the restart intervals; the bytes
// of the entropy segments, the interval table and the descriptors travel in one pinned blob and one async copy.  Three launches
// per call (k8_bgr or k8_nv12 by the output format), the picture in blockIdx.y (the grid covers the largest picture of the batch):
//   k8_entropy  one LANE per restart interval (a picture without DRI is one interval): Huffman decoding with libjpeg's scheme
//               (jdhuff.c: 8-bit look-ahead, maxcode / valoffset beyond), byte unstuffing, DC prediction from zero inside the
//               interval -> int16 coefficients in natural order, blocks in MCU order.  The picture's four tables sit in LDS.
//   k8_idct     one thread per 8x8 block: dequantise, jidctint.c "islow" (CONST_BITS 13, PASS1_BITS 2; columns, then rows), +128,
//               clamp -> the component's plane, padded to whole MCUs.
//   k8_bgr      one thread per pixel: fancy upsampling (jdsample.c h2v1 / h2v2 triangle filters over the component's REAL
//               downsampled size, edge rows and columns replicated; plain replication when that size is 2 columns or fewer, as
//               jinit_upsampler chooses) and jdcolor.c's 16-bit fixed-point YCbCr -> RGB.
//   k8_nv12     one thread per 2x2 pixels: Y' = 16 + (219 Y + 127) / 255, C' = 128 + (224 (C - 128) +- 127) / 255 (truncating), the
//               chroma pair the decoded 4:2:0 sample, the rounded mean of the two 4:2:2 rows or of the 2x2 4:4:4 group, 128 for gray.
// libjpeg's range-limit table WRAPS for IDCT sums outside [-512, 511] (before the +128) where these kernels saturate; streams
// from a real encoder never get there.  The tests use encoder-made streams and hand-built ones (tests/jpeg_craft.py: every table
// selection, 9..16-bit codes, block shapes and stuffing no encoder writes, each failure below on its own) that stay inside it.
//
// k8_entropy reads bytes from the outside world.  What keeps it in range whatever they hold:
//   * a byte is fetched only at pos < end of the lane's interval (K8Bits::fill); past the end the reader feeds zero bits and
//     counts them in `fake`, so the loops below never wait for data;
//   * the MCU count, the blocks per MCU and the 63 AC positions per block come from the descriptor, never from the bytes: every
//     loop has a fixed bound;
//   * a coefficient is stored at kNat[k] with k checked <= 63 first, inside the lane's own blocks;
//   * a symbol index is masked to the 256 entries of `vals`; a DC category is <= 15 by the host's check of the table, an AC
//     category by its 4 bits.
// What fails the picture (its flag is set, the lane ends):
//   * a code that is in no table: no length up to 16 has code <= maxcode[length];
//   * a run that passes index 63: k + run > 63 before a coefficient, or a ZRL that leaves k > 64;
//   * 0xFF inside the interval that 0x00 does not follow (the host cut the interval at every marker, so this is a broken stuffing
//     or a stream that ends in 0xFF);
//   * an interval that runs dry: after its last MCU more bits were taken than it had (fake > left);
//   * bytes left over: after its last MCU a byte is unread, or 8 or more real bits remain (less than a byte is padding).
#include "rva_internal.h"
#include "rva_jpeg_parse.h"

namespace {

struct K8Img {                              // one picture of a batch (the descriptor table)
    rva_jpeg_desc d;
    int32_t ok;                             // 0: refused by the parser -- no kernel touches it
    int32_t ival_first;                     // its first entry of the interval table
    int64_t bytes_off;                      // its entropy segment in the blob
    uint8_t *dst0, *dst1;
    int32_t pitch;
    int32_t bpm;                            // blocks per MCU
};

struct K8Args {
    const K8Img *img;
    const uint2 *ivals;
    const uint8_t *blob;
    int16_t *coef; size_t coef_img;         // [n][coef_img] int16: blocks in MCU order, natural order inside
    uint8_t *plane;                         // [n][coef_img] uint8: the component planes, one after the other
    int32_t *fail;                          // [n]
};

__constant__ uint8_t kNat[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                                 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                                 47, 55, 62, 63};

struct K8Bits {
    const uint8_t *p;
    uint32_t pos, end;
    unsigned long long acc;                 // the low `left` bits are unread, oldest on top
    int left, fake;                         // fake: zero bits fed past the interval's end (all at the bottom of acc)
    bool bad;                               // 0xFF without 0x00 after it

    __device__ __forceinline__ void fill()
    {
        while (left <= 56) {
            uint32_t b = 0;
            if (pos < end) {
                b = p[pos++];
                if (b == 0xFF) {
                    if (pos < end && p[pos] == 0) ++pos;
                    else bad = true;
                }
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            left += 8;
        }
    }
    __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)(acc >> (left - n)) & ((1u << n) - 1u); }   // 1 <= n <= 16 <= left
    __device__ __forceinline__ void skip(int n) { left -= n; }
};

// one Huffman symbol (jdhuff.c HUFF_DECODE): -1 if the next 16 bits start no code of the table
__device__ __forceinline__ int k8_symbol(K8Bits &br, const rva_jpeg_huff &h)
{
    br.fill();                              // >= 57 bits: a code (16) and its value bits (15) without another fill
    const uint32_t look = br.peek(8);
    int nb = h.look_nbits[look];
    if (nb) { br.skip(nb); return h.look_sym[look]; }
    for (nb = 9; nb <= 16; ++nb) {
        const int code = (int)br.peek(nb);
        if (code <= h.maxcode[nb]) { br.skip(nb); return h.vals[(code + h.valoff[nb]) & 255]; }
    }
    return -1;
}

__device__ __forceinline__ int k8_extend(K8Bits &br, int s)                    // s value bits -> the signed value (1 <= s <= 15)
{
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

__global__ void __launch_bounds__(64) k8_entropy(K8Args a)
{
    __shared__ rva_jpeg_huff huff[4];
    const int img = blockIdx.y;
    const K8Img &im = a.img[img];
    if (!im.ok) return;
    const int iv = blockIdx.x * 64 + threadIdx.x;
    if (blockIdx.x * 64 >= im.d.n_intervals) return;                          // the grid covers the picture with the most intervals
    {
        const uint32_t *src = (const uint32_t *)im.d.huff;
        uint32_t *dst = (uint32_t *)huff;
        for (int i = threadIdx.x; i < (int)(sizeof huff / 4); i += 64) dst[i] = src[i];
    }
    __syncthreads();
    if (iv >= im.d.n_intervals) return;
    const int n_mcu = im.d.mw * im.d.mh;
    const int per = im.d.restart_interval ? im.d.restart_interval : n_mcu;
    const int first = iv * per, last = min(first + per, n_mcu);                // the host checked n_intervals == ceil(n_mcu / per)
    const uint2 range = a.ivals[im.ival_first + iv];
    K8Bits br{a.blob + im.bytes_off, range.x, range.y, 0ull, 0, 0, false};
    const int bpm = im.bpm, luma = bpm == 1 ? 1 : bpm - 2;
    int16_t *coef = a.coef + (size_t)img * a.coef_img;
    int pred[3] = {0, 0, 0};
    bool fail = false;
    for (int m = first; m < last && !fail; ++m) {
        for (int k = 0; k < bpm && !fail; ++k) {
            const int c = k < luma ? 0 : k - luma + 1;
            const rva_jpeg_huff &dc = huff[im.d.dc_sel[c]], &ac = huff[im.d.ac_sel[c]];
            int16_t *blk = coef + ((size_t)m * bpm + k) * 64;
            for (int i = 0; i < 8; ++i) ((uint4 *)blk)[i] = make_uint4(0, 0, 0, 0);
            int s = k8_symbol(br, dc);
            if (s < 0) { fail = true; break; }                                 // a code in no table
            if (s) pred[c] = (int)((unsigned)pred[c] + (unsigned)k8_extend(br, s));
            blk[0] = (int16_t)pred[c];
            for (int kk = 1; kk < 64;) {
                const int rs = k8_symbol(br, ac);
                if (rs < 0) { fail = true; break; }                            // a code in no table
                const int r = rs >> 4;
                s = rs & 15;
                if (s) {
                    kk += r;
                    if (kk > 63) { fail = true; break; }                       // the run passes index 63
                    blk[kNat[kk]] = (int16_t)k8_extend(br, s);
                    ++kk;
                } else if (r == 15) {
                    kk += 16;
                    if (kk > 64) { fail = true; break; }                       // a ZRL that passes index 63
                } else {
                    break;                                                     // EOB
                }
            }
            if (br.bad) fail = true;                                           // 0xFF that 0x00 does not follow
        }
    }
    // ran dry: fake bits were consumed.  Left over: an unread byte, or a whole real byte still in the accumulator.
    if (!fail && (br.bad || br.fake > br.left || br.pos < br.end || br.left - br.fake >= 8)) fail = true;
    if (fail) atomicOr(a.fail + img, 1);
}

// jidctint.c jpeg_idct_islow, one 1-D pass.  COLS: pass 1 (from dequantised coefficients, results scaled by 2^PASS1_BITS);
// else pass 2 (descale by CONST_BITS + PASS1_BITS + 3).  64-bit sums: nothing a damaged stream holds overflows them.
template <bool COLS>
__device__ __forceinline__ void idct8(const int *in, int *out, int stride)
{
    typedef long long L;
    constexpr int SH = COLS ? 13 - 2 : 13 + 2 + 3;
    L z2 = in[2 * stride], z3 = in[6 * stride];
    L z1 = (z2 + z3) * 4433;
    L tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
    z2 = in[0]; z3 = in[4 * stride];
    L tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
    const L tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7 * stride]; tmp1 = in[5 * stride]; tmp2 = in[3 * stride]; tmp3 = in[stride];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    L z4 = tmp1 + tmp3;
    const L z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const L r = (L)1 << (SH - 1);
    out[0] = (int)((tmp10 + tmp3 + r) >> SH);
    out[7 * stride] = (int)((tmp10 - tmp3 + r) >> SH);
    out[stride] = (int)((tmp11 + tmp2 + r) >> SH);
    out[6 * stride] = (int)((tmp11 - tmp2 + r) >> SH);
    out[2 * stride] = (int)((tmp12 + tmp1 + r) >> SH);
    out[5 * stride] = (int)((tmp12 - tmp1 + r) >> SH);
    out[3 * stride] = (int)((tmp13 + tmp0 + r) >> SH);
    out[4 * stride] = (int)((tmp13 - tmp0 + r) >> SH);
}

// plane of component c: offset in the picture's plane scratch, width (its height is mh * (c ? 1 : vs) * 8)
__device__ __forceinline__ size_t k8_plane(const rva_jpeg_desc &d, int c, int &pw)
{
    const size_t luma = (size_t)d.mw * d.hs * 8 * d.mh * d.vs * 8, chroma = (size_t)d.mw * 8 * d.mh * 8;
    pw = c ? d.mw * 8 : d.mw * d.hs * 8;
    return c == 0 ? 0 : luma + (size_t)(c - 1) * chroma;
}

__global__ void __launch_bounds__(64) k8_idct(K8Args a)
{
    const int img = blockIdx.y;
    const K8Img &im = a.img[img];
    if (!im.ok) return;
    const rva_jpeg_desc &d = im.d;
    const int blk = blockIdx.x * 64 + threadIdx.x;
    const int bpm = im.bpm;
    if (blk >= d.mw * d.mh * bpm) return;
    const int mcu = blk / bpm, k = blk - mcu * bpm, my = mcu / d.mw, mx = mcu - my * d.mw;
    const int luma = bpm == 1 ? 1 : bpm - 2;
    const int c = k < luma ? 0 : k - luma + 1;
    const int bx = c == 0 ? mx * d.hs + k % d.hs : mx, by = c == 0 ? my * d.vs + k / d.hs : my;
    const int16_t *src = a.coef + (size_t)img * a.coef_img + (size_t)blk * 64;
    const uint16_t *q = d.q[c];
    int v[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) v[i] = (int)src[i] * (int)q[i];
#pragma unroll
    for (int col = 0; col < 8; ++col) idct8<true>(v + col, v + col, 8);
#pragma unroll
    for (int row = 0; row < 8; ++row) idct8<false>(v + 8 * row, v + 8 * row, 1);
    int pw;
    uint8_t *o = a.plane + (size_t)img * a.coef_img + k8_plane(d, c, pw) + (size_t)by * 8 * pw + bx * 8;
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        uint32_t w[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            w[h] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[h] |= (uint32_t)min(max(v[8 * row + 4 * h + j] + 128, 0), 255) << (8 * j);
        }
        *(uint2 *)(o + (size_t)row * pw) = make_uint2(w[0], w[1]);             // 8-byte aligned: pw and the block origin are multiples of 8
    }
}

// The upsampled chroma sample of plane `p` (width pw; real size cw x ch) at luma pixel (x, y): jdsample.c
__device__ __forceinline__ int k8_chroma(const uint8_t *p, int pw, int cw, int ch, int hs, int vs, int x, int y)
{
    if (hs == 1) return p[(size_t)y * pw + x];
    const int i = x >> 1;
    if (cw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * pw + i];            // jinit_upsampler: no triangle filter on so few columns
    const int in = min(max((x & 1) ? i + 1 : i - 1, 0), cw - 1);               // the horizontal neighbour, the edge column replicated
    if (vs == 1) {                                                             // h2v1: 3/4 near, 1/4 far; bias 1 (even) / 2 (odd)
        const uint8_t *row = p + (size_t)y * pw;
        if (in == i) return row[i];
        return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int r = y >> 1;
    const int rn = min(max((y & 1) ? r + 1 : r - 1, 0), ch - 1);               // the vertical neighbour, the edge row replicated
    const uint8_t *cur = p + (size_t)r * pw, *nb = p + (size_t)rn * pw;
    const int s = 3 * cur[i] + nb[i], sn = 3 * cur[in] + nb[in];
    return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ void __launch_bounds__(256) k8_bgr(K8Args a)
{
    const int img = blockIdx.y;
    const K8Img &im = a.img[img];
    if (!im.ok) return;
    const rva_jpeg_desc &d = im.d;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)d.width * d.height) return;
    const int y = (int)(idx / d.width), x = (int)(idx - (long long)y * d.width);
    const uint8_t *pl = a.plane + (size_t)img * a.coef_img;
    int pw;
    const int Y = pl[k8_plane(d, 0, pw) + (size_t)y * pw + x];
    int B = Y, G = Y, R = Y;
    if (d.ncomp == 3) {
        const int cw = (d.width + d.hs - 1) / d.hs, ch = (d.height + d.vs - 1) / d.vs;
        const size_t o1 = k8_plane(d, 1, pw), o2 = k8_plane(d, 2, pw);
        const int cb = k8_chroma(pl + o1, pw, cw, ch, d.hs, d.vs, x, y) - 128, cr = k8_chroma(pl + o2, pw, cw, ch, d.hs, d.vs, x, y) - 128;
        R = Y + ((91881 * cr + 32768) >> 16);                                  // jdcolor.c, SCALEBITS 16: FIX(1.40200)
        B = Y + ((116130 * cb + 32768) >> 16);                                 // FIX(1.77200)
        G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);                    // FIX(0.34414), FIX(0.71414)
        R = min(max(R, 0), 255); G = min(max(G, 0), 255); B = min(max(B, 0), 255);
    }
    uint8_t *o = im.dst0 + (size_t)y * im.pitch + 3 * (size_t)x;
    o[0] = (uint8_t)B; o[1] = (uint8_t)G; o[2] = (uint8_t)R;
}

__device__ __forceinline__ int k8_luma601(int y) { return 16 + (219 * y + 127) / 255; }
__device__ __forceinline__ int k8_chroma601(int c)
{
    const int v = 224 * (c - 128);
    return 128 + (v + (v < 0 ? -127 : 127)) / 255;                             // the division truncates
}

__global__ void __launch_bounds__(256) k8_nv12(K8Args a)
{
    const int img = blockIdx.y;
    const K8Img &im = a.img[img];
    if (!im.ok) return;
    const rva_jpeg_desc &d = im.d;
    const int qw = d.width >> 1, qh = d.height >> 1;                           // even sizes only (checked on the host)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)qw * qh) return;
    const int r = (int)(idx / qw), i = (int)(idx - (long long)r * qw);
    const uint8_t *pl = a.plane + (size_t)img * a.coef_img;
    int pw;
    const uint8_t *yp = pl + k8_plane(d, 0, pw);
    for (int dy = 0; dy < 2; ++dy) {
        const uint8_t *s = yp + (size_t)(2 * r + dy) * pw + 2 * i;
        uint8_t *o = im.dst0 + (size_t)(2 * r + dy) * im.pitch + 2 * i;
        o[0] = (uint8_t)k8_luma601(s[0]); o[1] = (uint8_t)k8_luma601(s[1]);
    }
    int c[2] = {128, 128};
    if (d.ncomp == 3)
        for (int k = 0; k < 2; ++k) {
            const uint8_t *p = pl + k8_plane(d, 1 + k, pw);
            if (d.hs == 2 && d.vs == 2) c[k] = p[(size_t)r * pw + i];
            else if (d.hs == 2) c[k] = (p[(size_t)(2 * r) * pw + i] + p[(size_t)(2 * r + 1) * pw + i] + 1) >> 1;
            else c[k] = (p[(size_t)(2 * r) * pw + 2 * i] + p[(size_t)(2 * r) * pw + 2 * i + 1] + p[(size_t)(2 * r + 1) * pw + 2 * i] +
                         p[(size_t)(2 * r + 1) * pw + 2 * i + 1] + 2) >> 2;
        }
    uint8_t *o = im.dst1 + (size_t)r * im.pitch + 2 * i;
    o[0] = (uint8_t)k8_chroma601(c[0]); o[1] = (uint8_t)k8_chroma601(c[1]);
}

void fill_info(const rva_jpeg_desc &d, rva_jpeg_dec_info *info)
{
    info->width = d.width; info->height = d.height; info->components = d.ncomp; info->h_samp = d.hs; info->v_samp = d.vs;
    info->restart_interval = d.restart_interval; info->intervals = d.n_intervals; info->mcus = d.mw * d.mh;
}

// 8x8 blocks a picture of up to w x h can hold, whatever its sampling
size_t max_blocks(int w, int h)
{
    const size_t w8 = (size_t)(w + 7) / 8, h8 = (size_t)(h + 7) / 8, w16 = (size_t)(w + 15) / 16, h16 = (size_t)(h + 15) / 16;
    return std::max({3 * w8 * h8, 4 * w16 * h8, 6 * w16 * h16});
}

}  // namespace

// The decoder object: every buffer a launch set touches, allocated once.
struct rva_jpeg_dec {
    rva_ctx *ctx = nullptr;
    int max_images = 0, max_w = 0, max_h = 0, max_bytes = 0;
    size_t max_ivals = 0;                   // per picture
    size_t off_ivals = 0, off_bytes = 0, blob_bytes = 0;      // the blob: [K8Img x max_images][uint2 x intervals in use][bytes]; sized for the most of each
    uint8_t *blob_host = nullptr, *blob_dev = nullptr;
    K8Args a{};
    int32_t *fail_host = nullptr;           // pinned [max_images]
    int8_t *refused = nullptr;              // [max_images] of the last call
    int last_n = 0;
    hipStream_t last_stream = nullptr;
    hipEvent_t uploaded = nullptr;          // the staging is free to rewrite once the previous call's copy has run
    hipEvent_t mark[5] = {};                // start, copied, entropy, idct, output of the last call (rva_jpeg_dec_times)
    bool timed = false;                     // the last call launched
};

extern "C" {

int rva_jpeg_dec_probe(const uint8_t *data, int64_t len, rva_jpeg_dec_info *info, char *msg, int msg_len)
{
    if (msg && msg_len > 0) msg[0] = 0;
    if (!data || len < 0 || !info) {
        if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "rva_jpeg_dec_probe: bad argument");
        return RVA_ERR_ARG;
    }
    static thread_local rva_jpeg_desc d;
    if (rva_jpeg::parse(data, (size_t)len, d, nullptr, 0, msg, msg_len > 0 ? (size_t)msg_len : 0)) return RVA_ERR_ARG;
    fill_info(d, info);
    return RVA_OK;
}

int rva_jpeg_dec_create(rva_ctx *ctx, int max_images, int max_width, int max_height, int max_bytes_per_image, rva_jpeg_dec **out)
{
    if (!ctx || !out || max_images < 1 || max_images > 4096 || max_width <= 0 || max_height <= 0 || max_width > 65535 || max_height > 65535 ||
        max_bytes_per_image < 16)
        return rva_fail(ctx, RVA_ERR_ARG, "rva_jpeg_dec_create: bad argument (1..4096 images of up to 65535x65535, >= 16 bytes each)");
    *out = nullptr;
    RVA_HIP(ctx, hipSetDevice(ctx->device));
    rva_jpeg_dec *e = new rva_jpeg_dec();
    e->ctx = ctx; e->max_images = max_images; e->max_w = max_width; e->max_h = max_height; e->max_bytes = max_bytes_per_image;
    const size_t n = (size_t)max_images;
    e->max_ivals = (size_t)((max_width + 7) / 8) * (size_t)((max_height + 7) / 8);        // one MCU per interval, 8x8 MCUs
    e->off_ivals = n * sizeof(K8Img);
    e->off_bytes = e->off_ivals + n * e->max_ivals * sizeof(uint2);
    e->blob_bytes = e->off_bytes + n * (((size_t)max_bytes_per_image + 15) & ~(size_t)15);
    e->a.coef_img = max_blocks(max_width, max_height) * 64;
    e->refused = new int8_t[n]();
    hipError_t err = hipMalloc(&e->blob_dev, e->blob_bytes);
    if (err == hipSuccess) err = hipHostMalloc(&e->blob_host, e->blob_bytes, hipHostMallocDefault);
    if (err == hipSuccess) err = hipMalloc(&e->a.coef, n * e->a.coef_img * sizeof(int16_t));
    if (err == hipSuccess) err = hipMalloc(&e->a.plane, n * e->a.coef_img);
    if (err == hipSuccess) err = hipMalloc(&e->a.fail, n * 4);
    if (err == hipSuccess) err = hipMemset(e->a.fail, 0, n * 4);
    if (err == hipSuccess) err = hipHostMalloc(&e->fail_host, n * 4, hipHostMallocDefault);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&e->uploaded, hipEventDisableTiming);
    for (int i = 0; i < 5 && err == hipSuccess; ++i) err = hipEventCreate(&e->mark[i]);
    if (err != hipSuccess) {
        rva_jpeg_dec_destroy(e);
        return rva_fail(ctx, RVA_ERR_HIP, "rva_jpeg_dec_create: %s (%d images of up to %dx%d)", hipGetErrorString(err), max_images, max_width,
                        max_height);
    }
    e->a.img = (const K8Img *)e->blob_dev;
    e->a.ivals = (const uint2 *)(e->blob_dev + e->off_ivals);
    e->a.blob = e->blob_dev;
    *out = e;
    return RVA_OK;
}

void rva_jpeg_dec_destroy(rva_jpeg_dec *e)
{
    if (!e) return;
    (void)hipSetDevice(e->ctx->device);
    (void)hipFree(e->blob_dev); (void)hipFree(e->a.coef); (void)hipFree(e->a.plane); (void)hipFree(e->a.fail);
    if (e->blob_host) (void)hipHostFree(e->blob_host);
    if (e->fail_host) (void)hipHostFree(e->fail_host);
    if (e->uploaded) (void)hipEventDestroy(e->uploaded);
    for (hipEvent_t m : e->mark)
        if (m) (void)hipEventDestroy(m);
    delete[] e->refused;
    delete e;
}

int rva_jpeg_dec_decode(rva_jpeg_dec *e, int n, const uint8_t *const *data, const int64_t *len, int format, void *const *dst0,
                        void *const *dst1, const int32_t *pitch, rva_stream_t stream)
{
    if (!e) return RVA_ERR_ARG;
    rva_ctx *ctx = e->ctx;
    const char *who = "rva_jpeg_dec_decode";
    if (!data || !len || !dst0 || !pitch || (format != RVA_JPEG_DEC_BGR && format != RVA_JPEG_DEC_NV12) || (format == RVA_JPEG_DEC_NV12 && !dst1))
        return rva_fail(ctx, RVA_ERR_ARG, "%s: bad argument (format BGR or NV12, NV12 takes dst1)", who);
    if (n < 1 || n > e->max_images) return rva_fail(ctx, RVA_ERR_ARG, "%s: %d images, the decoder was created for 1..%d", who, n, e->max_images);
    hipStream_t s = (hipStream_t)stream;
    RVA_HIP(ctx, hipSetDevice(ctx->device));
    RVA_HIP(ctx, hipEventSynchronize(e->uploaded));               // (returns at once unless a previous blob is still on its way)
    K8Img *tab = (K8Img *)e->blob_host;
    uint2 *ivals = (uint2 *)(e->blob_host + e->off_ivals);
    size_t n_ivals = 0;
    int top_ivals = 0;
    size_t top_blocks = 0, top_px = 0;
    bool first_refusal = true;
    char msg[256];
    for (int i = 0; i < n; ++i) {
        K8Img &im = tab[i];
        im.ok = 0; im.ival_first = 0; im.bytes_off = 0; im.dst0 = im.dst1 = nullptr; im.pitch = 0; im.bpm = 0;
        e->refused[i] = 1;
        int bad = !data[i] || len[i] < 0 ? rva_jpeg::refuse(msg, sizeof msg, "no data") :
                                           rva_jpeg::parse(data[i], (size_t)len[i], im.d, (uint32_t *)(ivals + n_ivals), e->max_ivals, msg, sizeof msg);
        const rva_jpeg_desc &d = im.d;
        if (!bad && (d.width > e->max_w || d.height > e->max_h))
            bad = rva_jpeg::refuse(msg, sizeof msg, "a picture of %dx%d, the decoder was created for up to %dx%d", d.width, d.height, e->max_w, e->max_h);
        if (!bad && d.scan_end - d.scan_begin > e->max_bytes)
            bad = rva_jpeg::refuse(msg, sizeof msg, "an entropy segment of %d bytes, the decoder was created for up to %d", d.scan_end - d.scan_begin,
                                   e->max_bytes);
        if (!bad && (size_t)d.n_intervals > e->max_ivals)                       // (cannot happen: an interval holds at least one MCU)
            bad = rva_jpeg::refuse(msg, sizeof msg, "%d restart intervals", d.n_intervals);
        if (bad) {
            im.d.n_intervals = 0;
            if (first_refusal) rva_fail(ctx, RVA_ERR_ARG, "%s: image %d refused: %s", who, i, msg);
            first_refusal = false;
            continue;
        }
        const int need = format == RVA_JPEG_DEC_BGR ? 3 * d.width : d.width;
        if (!dst0[i] || (format == RVA_JPEG_DEC_NV12 && !dst1[i]) || pitch[i] < need)
            return rva_fail(ctx, RVA_ERR_ARG, "%s: image %d (%dx%d) needs its destination and a pitch of at least %d bytes", who, i, d.width, d.height, need);
        if (format == RVA_JPEG_DEC_NV12 && ((d.width | d.height) & 1))
            return rva_fail(ctx, RVA_ERR_ARG, "%s: image %d is %dx%d, NV12 output takes even sizes only", who, i, d.width, d.height);
        e->refused[i] = 0;
        im.ok = 1; im.ival_first = (int32_t)n_ivals;
        im.dst0 = (uint8_t *)dst0[i]; im.dst1 = format == RVA_JPEG_DEC_NV12 ? (uint8_t *)dst1[i] : nullptr; im.pitch = pitch[i];
        im.bpm = d.ncomp == 1 ? 1 : d.hs * d.vs + 2;
        n_ivals += (size_t)d.n_intervals;
        top_ivals = std::max(top_ivals, d.n_intervals);
        top_blocks = std::max(top_blocks, (size_t)d.mw * d.mh * im.bpm);
        top_px = std::max(top_px, (size_t)d.width * d.height);
    }
    // the entropy segments follow the last interval that is in use, so that one copy of the blob's head carries all three
    size_t bytes = e->off_ivals + ((n_ivals * sizeof(uint2) + 15) & ~(size_t)15);
    for (int i = 0; i < n; ++i) {
        K8Img &im = tab[i];
        if (!im.ok) continue;
        const size_t nb = (size_t)(im.d.scan_end - im.d.scan_begin);
        im.bytes_off = (int64_t)bytes;
        memcpy(e->blob_host + bytes, data[i] + im.d.scan_begin, nb);
        bytes += (nb + 15) & ~(size_t)15;
    }
    e->last_n = n; e->last_stream = s;
    RVA_HIP(ctx, hipMemsetAsync(e->a.fail, 0, (size_t)n * 4, s));
    e->timed = top_ivals > 0;
    if (top_ivals) {
        RVA_HIP(ctx, hipEventRecord(e->mark[0], s));
        // one copy: the descriptors, the interval table and the bytes are one range of the blob
        RVA_HIP(ctx, hipMemcpyAsync(e->blob_dev, e->blob_host, bytes, hipMemcpyHostToDevice, s));
        RVA_HIP(ctx, hipEventRecord(e->uploaded, s));
        RVA_HIP(ctx, hipEventRecord(e->mark[1], s));
        const K8Args a = e->a;
        k8_entropy<<<dim3((unsigned)((top_ivals + 63) / 64), (unsigned)n), 64, 0, s>>>(a);
        RVA_HIP(ctx, hipEventRecord(e->mark[2], s));
        k8_idct<<<dim3((unsigned)((top_blocks + 63) / 64), (unsigned)n), 64, 0, s>>>(a);
        RVA_HIP(ctx, hipEventRecord(e->mark[3], s));
        if (format == RVA_JPEG_DEC_BGR) k8_bgr<<<dim3((unsigned)((top_px + 255) / 256), (unsigned)n), 256, 0, s>>>(a);
        else k8_nv12<<<dim3((unsigned)((top_px / 4 + 255) / 256), (unsigned)n), 256, 0, s>>>(a);
        RVA_HIP(ctx, hipEventRecord(e->mark[4], s));
        RVA_HIP(ctx, hipGetLastError());
    }
    RVA_HIP(ctx, hipMemcpyAsync(e->fail_host, e->a.fail, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    return RVA_OK;
}

int rva_jpeg_dec_status(rva_jpeg_dec *e, int32_t *status)
{
    if (!e || !status) return RVA_ERR_ARG;
    rva_ctx *ctx = e->ctx;
    RVA_HIP(ctx, hipSetDevice(ctx->device));
    RVA_HIP(ctx, hipStreamSynchronize(e->last_stream));
    for (int i = 0; i < e->last_n; ++i)
        status[i] = e->refused[i] ? RVA_JPEG_DEC_REFUSED : (e->fail_host[i] ? RVA_JPEG_DEC_FAILED : RVA_JPEG_DEC_OK);
    return RVA_OK;
}

int rva_jpeg_dec_times(rva_jpeg_dec *e, float *ms)
{
    if (!e || !ms) return RVA_ERR_ARG;
    rva_ctx *ctx = e->ctx;
    if (!e->timed) return rva_fail(ctx, RVA_ERR_ARG, "rva_jpeg_dec_times: the last decode launched nothing");
    RVA_HIP(ctx, hipSetDevice(ctx->device));
    RVA_HIP(ctx, hipEventSynchronize(e->mark[4]));
    for (int i = 0; i < 4; ++i) RVA_HIP(ctx, hipEventElapsedTime(ms + i, e->mark[i], e->mark[i + 1]));
    return RVA_OK;
}

}  // extern "C"
