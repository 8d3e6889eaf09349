// Host half of K8 (rva_jpeg_dec.hip): the marker walk of a baseline JPEG stream.  Plain C++ that includes nothing of HIP, so that
// tools/jpeg_parse_check.cpp can compile it alone under a sanitizer.  It takes bytes from the outside world: every read is
// checked against the end of the stream first (Reader / the explicit `i + 1 < len` tests of the scan), every table index against
// its table, and nothing is allocated.
//
// rva_jpeg_parse() fills an rva_jpeg_desc -- geometry, sampling, the four Huffman tables in libjpeg's decode form (jdhuff.c
// jpeg_make_d_derived_tbl: an 8-bit look-ahead table plus maxcode / valoffset for longer codes), the dequantisation tables in
// natural order -- and the byte range of every restart interval of the entropy segment (an image without DRI is one interval).
//
// Accepted: SOF0, 8-bit samples, Huffman coding, ONE interleaved scan; 1 component, or Y/Cb/Cr with chroma 1x1 and luma 1x1
// (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0); 8-bit DQT, ids 0..3; any DHT (ids 0 and 1); a table defined again (the last definition
// before SOS holds) and several tables in one segment; tables and DRI before or after SOF0; optional DRI (the last one holds, 0
// or a count >= the MCUs: one interval); fill 0xFF in front of any marker; APPn / COM of any content (skipped by their length).
// The colour space of three components follows libjpeg's default_decompress_parms, which is what cv2.imdecode and Pillow show:
// a JFIF APP0 says YCbCr; else an Adobe APP14 decides by its transform (1: YCbCr); else component ids 1,2,3 are YCbCr, ids
// 'R','G','B' are RGB samples, any other ids YCbCr.  RGB samples are refused (there is no colour conversion to leave out here),
// and so is every Adobe transform but 1, also beside a JFIF marker, where libjpeg would believe JFIF: the two contradict each
// other.  Everything else is refused with a message that names what was found.
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

struct rva_jpeg_huff {                     // one Huffman table in decode form
    uint8_t look_nbits[256];               // code length of the symbol the next 8 bits start with, 0: the code is longer than 8 bits
    uint8_t look_sym[256];
    int32_t maxcode[18];                   // [l] largest code of length l (-1: none); [17] = 0xFFFFF ends every search
    int32_t valoff[17];                    // [l] index into vals of the first code of length l, minus that code
    uint8_t vals[256];
};

struct rva_jpeg_desc {
    int32_t width, height, ncomp;
    int32_t hs, vs;                        // luma sampling factors (chroma is 1x1); 1, 1 for a grayscale stream
    int32_t mw, mh;                        // MCUs per row / rows of MCUs
    int32_t restart_interval;              // MCUs per restart interval as DRI says, 0: none
    int32_t n_intervals;                   // restart intervals of the scan (1 without DRI)
    int32_t scan_begin, scan_end;          // byte range of the entropy segment in the stream (scan_end: the marker that ends it)
    int32_t dc_sel[3], ac_sel[3];          // per component: which of huff[0..1] (DC) / huff[2..3] (AC)
    uint16_t q[3][64];                     // per component: dequantisation table, natural order
    rva_jpeg_huff huff[4];                 // DC 0, DC 1, AC 0, AC 1
};

namespace rva_jpeg {

constexpr uint8_t kNatural[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                                  28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                                  47, 55, 62, 63};

inline int refuse(char *msg, size_t msg_len, const char *fmt, ...)
{
    if (msg && msg_len) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, msg_len, fmt, ap);
        va_end(ap);
    }
    return 1;
}

// jdhuff.c jpeg_make_d_derived_tbl.  counts[16]: codes per length 1..16; nsym symbols.  Returns nullptr or what is wrong.
inline const char *derive_huff(const uint8_t *counts, const uint8_t *syms, int nsym, bool is_dc, rva_jpeg_huff &h)
{
    uint8_t size[257];
    uint32_t codes[257];
    int p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < counts[l - 1]; ++i) size[p++] = (uint8_t)l;        // p <= nsym <= 256: the caller summed the counts
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        while (k < p && size[k] == l) codes[k++] = code++;
        if (code > (1u << l)) return "codes overflow their length";
        code <<= 1;
    }
    memset(&h, 0, sizeof h);
    k = 0;
    for (int l = 1; l <= 16; ++l) {
        if (counts[l - 1]) {
            h.valoff[l] = k - (int32_t)codes[k];
            k += counts[l - 1];
            h.maxcode[l] = (int32_t)codes[k - 1];
        } else {
            h.maxcode[l] = -1;
        }
    }
    h.maxcode[0] = -1;
    h.maxcode[17] = 0xFFFFF;
    k = 0;
    for (int l = 1; l <= 8; ++l)
        for (int i = 0; i < counts[l - 1]; ++i, ++k) {
            const int first = (int)(codes[k] << (8 - l));                      // codes[k] < 2^l (checked above): first + span <= 256
            for (int j = 0; j < (1 << (8 - l)); ++j) {
                h.look_nbits[first + j] = (uint8_t)l;
                h.look_sym[first + j] = syms[k];
            }
        }
    for (int i = 0; i < nsym; ++i) {
        if (is_dc && syms[i] > 15) return "a DC symbol above 15";
        h.vals[i] = syms[i];
    }
    return nullptr;
}

inline const char *sof_name(int m)
{
    switch (m) {
    case 0xC1: return "SOF1 (extended sequential)";
    case 0xC2: return "SOF2 (progressive)";
    case 0xC3: return "SOF3 (lossless)";
    case 0xC5: case 0xC6: case 0xC7: return "SOF5..7 (differential)";
    default: return "SOF9..15 (arithmetic coding)";
    }
}

// The marker walk.  `ivals` (may be null) receives up to ival_cap (begin, end) byte offsets, relative to d.scan_begin, one pair
// per restart interval; d.n_intervals counts all of them either way.  Returns 0, or 1 with the refusal in msg.
inline int parse(const uint8_t *s, size_t len, rva_jpeg_desc &d, uint32_t *ivals, size_t ival_cap, char *msg, size_t msg_len)
{
    memset(&d, 0, sizeof d);
    if (msg && msg_len) msg[0] = 0;
    if (!s || len < 4 || s[0] != 0xFF || s[1] != 0xD8) return refuse(msg, msg_len, "not a JPEG stream (no SOI)");
    if (len > 0x7FFFFFF0u) return refuse(msg, msg_len, "a stream of %zu bytes (2 GiB at the most)", len);
    uint16_t qt[4][64];
    bool have_q[4] = {}, have_h[4] = {}, have_sof = false;
    int comp_id[3] = {}, comp_tq[3] = {}, adobe = -1;
    bool jfif = false;
    size_t p = 2;
    for (;;) {
        // a marker: 0xFF, any number of fill 0xFF, the code
        if (p >= len) return refuse(msg, msg_len, "the stream ends before SOS");
        if (s[p] != 0xFF) return refuse(msg, msg_len, "byte 0x%02x at offset %zu where a marker should be", s[p], p);
        while (p < len && s[p] == 0xFF) ++p;
        if (p >= len) return refuse(msg, msg_len, "the stream ends inside a marker");
        const int m = s[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;                 // no payload
        if (m == 0xD9) return refuse(msg, msg_len, "EOI before SOS");
        if (m == 0x00) return refuse(msg, msg_len, "stuffed zero outside a scan at offset %zu", p - 1);
        if (p + 2 > len) return refuse(msg, msg_len, "the stream ends inside marker segment 0x%02x", m);
        const size_t seg = ((size_t)s[p] << 8) | s[p + 1];
        if (seg < 2) return refuse(msg, msg_len, "marker segment 0x%02x with length %zu", m, seg);
        if (p + seg > len) return refuse(msg, msg_len, "the stream ends inside marker segment 0x%02x", m);
        const uint8_t *b = s + p + 2;                                                  // payload: n bytes, all inside the stream
        const size_t n = seg - 2;
        p += seg;
        if (m == 0xC0) {
            if (have_sof) return refuse(msg, msg_len, "a second SOF0");
            if (n < 6) return refuse(msg, msg_len, "SOF0 of %zu bytes", n);
            if (b[0] != 8) return refuse(msg, msg_len, "%d-bit samples (8-bit only)", b[0]);
            d.height = (b[1] << 8) | b[2]; d.width = (b[3] << 8) | b[4]; d.ncomp = b[5];
            if (d.height == 0) return refuse(msg, msg_len, "height 0 (the number of lines comes in a DNL marker)");
            if (d.width == 0) return refuse(msg, msg_len, "width 0");
            if (d.ncomp != 1 && d.ncomp != 3) return refuse(msg, msg_len, "%d components (1 or 3 only)", d.ncomp);
            if (n != (size_t)(6 + 3 * d.ncomp)) return refuse(msg, msg_len, "SOF0 of %zu bytes for %d components", n, d.ncomp);
            int h[3], v[3];
            for (int c = 0; c < d.ncomp; ++c) {
                comp_id[c] = b[6 + 3 * c]; h[c] = b[7 + 3 * c] >> 4; v[c] = b[7 + 3 * c] & 15; comp_tq[c] = b[8 + 3 * c];
                if (comp_tq[c] > 3) return refuse(msg, msg_len, "quantisation table id %d", comp_tq[c]);
                if (h[c] < 1 || h[c] > 4 || v[c] < 1 || v[c] > 4) return refuse(msg, msg_len, "sampling factors %dx%d", h[c], v[c]);
            }
            d.hs = d.vs = 1;                                                           // one component: the scan is not interleaved
            if (d.ncomp == 3) {
                const bool luma_ok = (h[0] == 1 && v[0] == 1) || (h[0] == 2 && v[0] == 1) || (h[0] == 2 && v[0] == 2);
                if (!luma_ok || h[1] != 1 || v[1] != 1 || h[2] != 1 || v[2] != 1)
                    return refuse(msg, msg_len, "sampling factors %dx%d %dx%d %dx%d (4:4:4, 4:2:2 and 4:2:0 only)", h[0], v[0], h[1], v[1],
                                  h[2], v[2]);
                d.hs = h[0]; d.vs = v[0];
            }
            d.mw = (d.width + 8 * d.hs - 1) / (8 * d.hs); d.mh = (d.height + 8 * d.vs - 1) / (8 * d.vs);
            have_sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return refuse(msg, msg_len, "%s: baseline SOF0 only", sof_name(m));
        } else if (m == 0xCC) {
            return refuse(msg, msg_len, "DAC (arithmetic coding): baseline SOF0 only");
        } else if (m == 0xDB) {
            for (size_t i = 0; i < n;) {
                const int pq = b[i] >> 4, tq = b[i] & 15;
                if (pq != 0) return refuse(msg, msg_len, "16-bit DQT (8-bit tables only)");
                if (tq > 3) return refuse(msg, msg_len, "DQT table id %d", tq);
                if (i + 65 > n) return refuse(msg, msg_len, "the stream ends inside marker segment 0xdb (a table of %zu bytes)", n - i - 1);
                for (int k = 0; k < 64; ++k) qt[tq][kNatural[k]] = b[i + 1 + k];
                have_q[tq] = true;
                i += 65;
            }
        } else if (m == 0xC4) {
            for (size_t i = 0; i < n;) {
                const int tc = b[i] >> 4, th = b[i] & 15;
                if (tc > 1 || th > 1) return refuse(msg, msg_len, "DHT class %d id %d (baseline: class 0..1, id 0..1)", tc, th);
                if (i + 17 > n) return refuse(msg, msg_len, "the stream ends inside marker segment 0xc4 (counts)");
                int nsym = 0;
                for (int k = 0; k < 16; ++k) nsym += b[i + 1 + k];
                if (nsym > 256) return refuse(msg, msg_len, "DHT counts overflow 256 symbols (%d)", nsym);
                if (i + 17 + (size_t)nsym > n) return refuse(msg, msg_len, "the stream ends inside marker segment 0xc4 (symbols)");
                const char *bad = derive_huff(b + i + 1, b + i + 17, nsym, tc == 0, d.huff[2 * tc + th]);
                if (bad) return refuse(msg, msg_len, "DHT class %d id %d: %s", tc, th, bad);
                have_h[2 * tc + th] = true;
                i += 17 + (size_t)nsym;
            }
        } else if (m == 0xDD) {
            if (n != 2) return refuse(msg, msg_len, "DRI of %zu bytes", n);
            d.restart_interval = (b[0] << 8) | b[1];
        } else if (m == 0xDC) {
            return refuse(msg, msg_len, "DNL marker (the number of lines must be in SOF0)");
        } else if (m == 0xEE && n >= 12 && memcmp(b, "Adobe", 5) == 0) {
            adobe = b[11];
        } else if (m == 0xE0 && n >= 14 && memcmp(b, "JFIF", 5) == 0) {                  // (libjpeg's lengths: examine_app0 / examine_app14)
            jfif = true;
        } else if (m == 0xDA) {
            if (!have_sof) return refuse(msg, msg_len, "SOS before SOF0");
            if (n < 1) return refuse(msg, msg_len, "SOS of 0 bytes");
            const int ns = b[0];
            if (ns != d.ncomp)
                return refuse(msg, msg_len, "a scan of %d of the frame's %d components (several scans: one interleaved scan only)", ns, d.ncomp);
            if (n != (size_t)(4 + 2 * ns)) return refuse(msg, msg_len, "SOS of %zu bytes for %d components", n, ns);
            for (int c = 0; c < ns; ++c) {
                if (b[1 + 2 * c] != comp_id[c]) return refuse(msg, msg_len, "scan component %d is not frame component %d", b[1 + 2 * c], comp_id[c]);
                const int td = b[2 + 2 * c] >> 4, ta = b[2 + 2 * c] & 15;
                if (td > 1 || ta > 1) return refuse(msg, msg_len, "Huffman table ids %d/%d (baseline: 0..1)", td, ta);
                if (!have_h[td]) return refuse(msg, msg_len, "missing DC Huffman table %d", td);
                if (!have_h[2 + ta]) return refuse(msg, msg_len, "missing AC Huffman table %d", ta);
                if (!have_q[comp_tq[c]]) return refuse(msg, msg_len, "missing quantisation table %d", comp_tq[c]);
                d.dc_sel[c] = td; d.ac_sel[c] = 2 + ta;
                memcpy(d.q[c], qt[comp_tq[c]], sizeof d.q[c]);
            }
            if (b[1 + 2 * ns] != 0 || b[2 + 2 * ns] != 63 || b[3 + 2 * ns] != 0)
                return refuse(msg, msg_len, "scan parameters Ss %d Se %d AhAl 0x%02x (progressive; sequential is 0 63 0)", b[1 + 2 * ns],
                              b[2 + 2 * ns], b[3 + 2 * ns]);
            if (d.ncomp == 3 && adobe == 0) return refuse(msg, msg_len, "Adobe transform 0 (RGB samples; YCbCr only)");
            if (d.ncomp == 3 && adobe > 1) return refuse(msg, msg_len, "Adobe transform %d (YCbCr only)", adobe);
            if (d.ncomp == 3 && !jfif && adobe < 0 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
                return refuse(msg, msg_len, "component ids 'R','G','B' without a JFIF or Adobe marker (RGB samples; YCbCr only)");
            break;
        }
        // every other segment (APPn, COM, ...) is skipped by its length: an embedded thumbnail cannot be taken for the frame
    }
    // the entropy segment: 0xFF is followed by 0x00 (a stuffed data byte), 0xFF (fill), RSTn (the interval ends) or the marker
    // that ends the scan.  A stream that ends without one is taken to its last byte: the device then finds the interval dry.
    d.scan_begin = (int32_t)p;
    const long long mcus = (long long)d.mw * d.mh;
    const long long want = d.restart_interval ? (mcus + d.restart_interval - 1) / d.restart_interval : 1;
    size_t begin = p, i = p;
    long long count = 0;
    int end_marker = -1;
    for (;;) {
        while (i < len && s[i] != 0xFF) ++i;
        size_t end = i;                                                                // the interval's bytes are [begin, end)
        if (i < len) {
            size_t j = i;
            while (j < len && s[j] == 0xFF) ++j;                                       // fill bytes belong to the marker
            if (j < len && s[j] == 0x00 && j == i + 1) { i += 2; continue; }           // 0xFF 0x00: data
            if (j < len && s[j] == 0x00) { i = j - 1; continue; }                      // fill, then a stuffed 0xFF: leave it to the device (it fails the interval)
            if (j >= len) { end = len; i = len; }                                      // the stream ends in 0xFF: a data byte with nothing after it
            else { end_marker = s[j]; i = j + 1; }
        }
        if (ivals && (size_t)count < ival_cap) {
            ivals[2 * count] = (uint32_t)(begin - p);
            ivals[2 * count + 1] = (uint32_t)(end - p);
        }
        ++count;
        if (end_marker >= 0xD0 && end_marker <= 0xD7) {
            if (!d.restart_interval) return refuse(msg, msg_len, "RST%d in a scan without DRI", end_marker - 0xD0);
            if (end_marker - 0xD0 != (int)((count - 1) & 7))
                return refuse(msg, msg_len, "RST%d where RST%d is due", end_marker - 0xD0, (int)((count - 1) & 7));
            if (count >= want) return refuse(msg, msg_len, "more than the %lld restart intervals of %d MCUs that %lld MCUs need", want, d.restart_interval, mcus);
            begin = i;
            end_marker = -1;
            continue;
        }
        d.scan_end = (int32_t)end;
        break;
    }
    if (end_marker == 0xDA) return refuse(msg, msg_len, "a second SOS (several scans: one interleaved scan only)");
    if (end_marker == 0xDC) return refuse(msg, msg_len, "DNL marker after the scan");
    if (end_marker >= 0 && end_marker != 0xD9) return refuse(msg, msg_len, "marker 0x%02x after the scan where EOI should be", end_marker);
    if (count != want) return refuse(msg, msg_len, "%lld restart intervals where %lld MCUs in intervals of %d need %lld", count, mcus, d.restart_interval, want);
    d.n_intervals = (int32_t)count;
    return 0;
}

}  // namespace rva_jpeg
