"""A compact numpy decoder for baseline JPEG, the arithmetic of libjpeg restated step by step: Huffman decoding, dequantisation,
jidctint.c's islow IDCT, jdsample.c's fancy upsampling, jdcolor.c's colour conversion.  tests/test_jpeg_dec_host.py asserts its RGB
equal to Pillow's libjpeg-turbo on the whole stream grid, which makes its intermediate planes a trustworthy source for what K8's
NV12 output must be (there is no other reference for that).  Also the stream makers the K8 tests share."""
import io

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

SIZES = [(1, 1), (8, 8), (16, 16), (17, 13), (33, 47), (40, 48), (15, 34)]          # (width, height)
SAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}                                    # Pillow's `subsampling`
QUALITIES = [5, 50, 90, 100]
RESTARTS = [0, 1, 3]                                                                # restart_marker_blocks (MCUs per interval)


def make_image(w, h, seed, ramp=False):
    """RGB uint8 [h, w, 3]: seeded noise over a gradient, or (ramp) a smooth ramp whose blocks are long zero runs and EOBs."""
    yy, xx = np.mgrid[0:h, 0:w]
    if ramp:
        return np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)
    rng = np.random.default_rng(seed)
    base = np.stack([xx * 5 + 20, yy * 4 + 40, (xx + yy) * 3], -1) % 256
    return ((base + rng.integers(-60, 61, (h, w, 3))) % 256).astype(np.uint8)


def encode(img, quality=90, subsampling=2, **kw):
    from PIL import Image
    buf = io.BytesIO()
    im = Image.fromarray(img)
    if im.mode == "L":
        im.save(buf, "JPEG", quality=quality, **kw)
    else:
        im.save(buf, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def grid(qualities=QUALITIES, restarts=RESTARTS):
    """(id, bytes) of the stream grid: sizes x sampling x quality x restart, each size once as noise and (quality 90) as a ramp."""
    for w, h in SIZES:
        for name, sub in SAMPLINGS.items():
            for q in qualities:
                for r in restarts:
                    kw = {"restart_marker_blocks": r} if r else {}
                    ramp = q == 90
                    yield f"{w}x{h}-{name}-q{q}-r{r}", encode(make_image(w, h, 1000 + w * 7 + h, ramp=ramp), q, sub, **kw)


# ------------------------------------------------------------------------------------------ the decoder
class _Bits:
    def __init__(self, data):
        out, i = bytearray(), 0
        while i < len(data):                       # unstuff
            out.append(data[i])
            i += 2 if data[i] == 0xFF else 1
        self.d, self.pos, self.n = bytes(out), 0, len(out) * 8

    def get(self, k):
        v = 0
        for _ in range(k):
            assert self.pos < self.n, "interval ran dry"
            v = (v << 1) | ((self.d[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v


def _huff_table(counts, syms):
    tbl, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            tbl[(length, code)] = syms[k]
            code += 1
            k += 1
        code <<= 1
    return tbl


def _symbol(br, tbl, longest=16):
    code = 0
    for length in range(1, longest + 1):
        code = (code << 1) | br.get(1)
        if (length, code) in tbl:
            return tbl[(length, code)]
    raise AssertionError("code in no table")


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


FAULTS = ("ac-by-dc-id", "q-min-c-1", "cb-cr-swapped", "first-definition", "first-of-segment", "pred-kept", "zrl-64-error", "search-15")


def parse(data, fault=None):
    """Markers of a baseline stream -> dict(w, h, comps [(id, h, v, tq)], q {id: [64] natural}, huff {(class, id): table}, ri,
    sel [(td, ta)], intervals [bytes]).  Any number of fill 0xFF may stand in front of a marker, in the header and in the scan.
    `fault` plants one of FAULTS (tests/test_jpeg_craft_host.py: what a decoder gets wrong without the stream grid noticing)."""
    assert data[:2] == b"\xff\xd8"
    p, q, huff, ri, frame = 2, {}, {}, 0, None
    while True:
        assert data[p] == 0xFF
        while data[p + 1] == 0xFF:
            p += 1
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        b = data[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xDB:
            while b:
                assert b[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(b[1:65])
                if not (fault == "first-definition" and b[0] & 15 in q):
                    q[b[0] & 15] = t
                b = b[65:] if fault != "first-of-segment" else b""
        elif m == 0xC4:
            while b:
                counts = list(b[1:17])
                if not (fault == "first-definition" and (b[0] >> 4, b[0] & 15) in huff):
                    huff[(b[0] >> 4, b[0] & 15)] = _huff_table(counts, list(b[17:17 + sum(counts)]))
                b = b[17 + sum(counts):] if fault != "first-of-segment" else b""
        elif m == 0xC0:
            assert b[0] == 8
            frame = dict(h=(b[1] << 8) | b[2], w=(b[3] << 8) | b[4],
                         comps=[(b[6 + 3 * c], b[7 + 3 * c] >> 4, b[7 + 3 * c] & 15, b[8 + 3 * c]) for c in range(b[5])])
        elif m == 0xDD:
            ri = (b[0] << 8) | b[1]
        elif m == 0xDA:
            sel = [(b[2 + 2 * c] >> 4, b[2 + 2 * c] & 15) for c in range(b[0])]
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC9, 0xCA), "not baseline"
    intervals, start, i = [], p, p
    while True:
        if data[i] == 0xFF and data[i + 1] != 0:
            intervals.append(data[start:i])
            while data[i + 1] == 0xFF:             # fill bytes belong to the marker
                i += 1
            if 0xD0 <= data[i + 1] <= 0xD7:
                i += 2
                start = i
                continue
            break
        i += 2 if data[i] == 0xFF else 1
    return dict(frame, q=q, huff=huff, ri=ri, sel=sel, intervals=intervals)


def _idct_1d(x, shift):
    """jidctint.c, one pass over the leading axis of x [8, ...] (int64)."""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 + z3 * -15137, z1 + z2 * 6270
    tmp0, tmp1 = (x[0] + x[4]) << 13, (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]) + r >> shift


def idct_raw(block):
    """Dequantised coefficients [8, 8] (natural order) -> the IDCT's output before the level shift and the clamp."""
    ws = _idct_1d(block.astype(np.int64), 11)             # columns: rows of the array are the vertical frequency
    return _idct_1d(ws.T, 18).T                           # rows


def idct(block):
    """Dequantised coefficients [8, 8] (natural order) -> samples 0..255."""
    return np.clip(idct_raw(block) + 128, 0, 255)


def _fancy_h(a, even_bias, odd_bias, shift, w3):
    """The horizontal triangle filter of jdsample.c over rows `a` [rows, cw] (cw > 2): 2 cw columns."""
    left = np.concatenate([a[:, :1], a[:, :-1]], 1)
    right = np.concatenate([a[:, 1:], a[:, -1:]], 1)
    out = np.empty((a.shape[0], 2 * a.shape[1]), np.int64)
    out[:, 0::2] = (w3 * a + left + even_bias) >> shift
    out[:, 1::2] = (w3 * a + right + odd_bias) >> shift
    return out


def upsample(plane, hs, vs, w, h):
    """A chroma plane (padded) -> [h, w] at luma resolution.  The counts are the component's real size, ceil(w / hs) x ceil(h / vs);
    2 columns or fewer are replicated (jinit_upsampler uses the triangle filters only above that)."""
    if hs == 1:
        return plane[:h, :w].astype(np.int64)
    cw, ch = -(-w // hs), -(-h // vs)
    a = plane[:ch, :cw].astype(np.int64)
    if cw <= 2:
        return np.repeat(np.repeat(a, vs, 0), 2, 1)[:h, :w]
    if vs == 1:
        out = _fancy_h(a, 1, 2, 2, 3)
        out[:, 0], out[:, -1] = a[:, 0], a[:, -1]
        return out[:h, :w]
    up = np.concatenate([a[:1], a[:-1]], 0)
    down = np.concatenate([a[1:], a[-1:]], 0)
    s = np.empty((2 * ch, cw), np.int64)
    s[0::2], s[1::2] = 3 * a + up, 3 * a + down
    return _fancy_h(s, 8, 7, 4, 3)[:h, :w]


def decode(data, fault=None):
    """-> dict(w, h, ncomp, hs, vs, planes [Y(, Cb, Cr)] padded to whole MCUs, rgb [h, w, 3] uint8).  `fault`: see parse()."""
    assert fault is None or fault in FAULTS
    f = parse(data, fault)
    w, h, comps = f["w"], f["h"], f["comps"]
    nc = len(comps)
    sel, tq = list(f["sel"]), [c[3] for c in comps]
    if fault == "ac-by-dc-id":
        sel = [(td, td) for td, _ in sel]
    if fault == "q-min-c-1":
        tq = [tq[min(c, 1)] for c in range(nc)]
    if fault == "cb-cr-swapped" and nc == 3:
        sel, tq = [sel[0], sel[2], sel[1]], [tq[0], tq[2], tq[1]]
    longest = 15 if fault == "search-15" else 16
    hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    planes = [np.zeros((mh * vs * 8, mw * hs * 8), np.int64)] + [np.zeros((mh * 8, mw * 8), np.int64) for _ in range(nc - 1)]
    per = f["ri"] or mw * mh
    assert len(f["intervals"]) == -(-mw * mh // per)
    pred = [0] * nc
    for iv, seg in enumerate(f["intervals"]):
        br = _Bits(seg)
        if fault != "pred-kept":
            pred = [0] * nc
        for mcu in range(iv * per, min((iv + 1) * per, mw * mh)):
            my, mx = divmod(mcu, mw)
            for c in range(nc):
                dc, ac = f["huff"][(0, sel[c][0])], f["huff"][(1, sel[c][1])]
                for k in range(hs * vs if c == 0 else 1):
                    coef = np.zeros(64, np.int64)
                    s = _symbol(br, dc, longest)
                    pred[c] += _extend(br.get(s), s) if s else 0
                    coef[0] = pred[c]
                    i = 1
                    while i < 64:
                        rs = _symbol(br, ac, longest)
                        r, s = rs >> 4, rs & 15
                        if s:
                            i += r
                            coef[ZIGZAG[i]] = _extend(br.get(s), s)
                            i += 1
                        elif r == 15:
                            i += 16
                            assert i <= 64 and not (fault == "zrl-64-error" and i == 64), "a ZRL passes index 63"
                        else:
                            break
                    by, bx = (my * vs + k // hs, mx * hs + k % hs) if c == 0 else (my, mx)
                    planes[c][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = idct((coef * f["q"][tq[c]]).reshape(8, 8))
    y = planes[0][:h, :w]
    if nc == 1:
        rgb = np.stack([y, y, y], -1)
    else:
        cb, cr = upsample(planes[1], hs, vs, w, h) - 128, upsample(planes[2], hs, vs, w, h) - 128
        r = y + ((91881 * cr + 32768) >> 16)
        b = y + ((116130 * cb + 32768) >> 16)
        g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
        rgb = np.clip(np.stack([r, g, b], -1), 0, 255)
    return dict(w=w, h=h, ncomp=nc, hs=hs, vs=vs, planes=planes, rgb=rgb.astype(np.uint8))


def nv12_expected(dec):
    """K8's NV12 definition applied to the decoder's planes: (Y' [h, w], CbCr' [h / 2, w] interleaved), BT.601 limited range."""
    w, h, hs, vs = dec["w"], dec["h"], dec["hs"], dec["vs"]
    assert w % 2 == 0 and h % 2 == 0
    y = 16 + (219 * dec["planes"][0][:h, :w] + 127) // 255
    uv = np.full((h // 2, w), 128, np.int64)
    if dec["ncomp"] == 3:
        for k in range(2):
            p = dec["planes"][1 + k]
            if (hs, vs) == (2, 2):
                c = p[:h // 2, :w // 2]
            elif (hs, vs) == (2, 1):
                c = (p[0:h:2, :w // 2] + p[1:h:2, :w // 2] + 1) >> 1
            else:
                c = (p[0:h:2, 0:w:2] + p[0:h:2, 1:w:2] + p[1:h:2, 0:w:2] + p[1:h:2, 1:w:2] + 2) >> 2
            v = 224 * (c - 128)
            uv[:, k::2] = 128 + np.sign(v) * ((np.abs(v) + 127) // 255)          # truncating division, the 127 with the sign of v
    return y.astype(np.uint8), uv.astype(np.uint8)
