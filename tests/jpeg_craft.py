"""A baseline-JPEG writer for tests: quantised coefficient blocks in, a legal SOF0 stream out, with everything a real encoder never
varies as a parameter -- the Huffman tables and which component uses which, the quantisation tables and their ids, the component
ids, the layout of the marker segments, DRI, fill bytes, the padding bit -- and hooks that make a stream wrong in exactly one way.
write() also returns facts about the stream it made (stuffed bytes, code lengths), so that a test can assert that a stream has the
property it was built for.  tests/test_jpeg_craft_host.py pins every stream used on the GPU to Pillow through tests/jpeg_ref.py.

Blocks stay inside the range where libjpeg and jpeg_ref agree by construction: the IDCT's output before the +128 lies in
[-512, 511] (the span libjpeg's range-limit table maps to saturation; beyond it libjpeg wraps and K8 saturates), DC differences
within +-2047 and AC coefficients within +-1023 (the categories baseline Huffman coding has)."""
import numpy as np

from tests import jpeg_ref as J

AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]          # EOB, ZRL, run/size: all 162 of baseline
ONES = [1] * 64


def flat(symbols, length):
    """A table whose codes all have one length."""
    counts = [0] * 16
    counts[length - 1] = len(symbols)
    return counts, list(symbols)


def codes(table):
    """(counts[16], symbols) -> {symbol: (code, length)}, the canonical assignment of a DHT segment."""
    counts, symbols = table
    assert len(counts) == 16 and sum(counts) == len(symbols) == len(set(symbols)) <= 256
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            assert code < (1 << length) - 1, "the all-ones code is never used"
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


# Annex K's code lengths.  DC0 / DC1 and AC0 / AC1 give the same symbol different codes, so a component read with the other table
# decodes to something else (or to nothing).
DC0 = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC1 = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(11, -1, -1)))
AC0 = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], AC_SYMBOLS)
AC1 = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [0x00] + AC_SYMBOLS[:0:-1])
# no code of 8 bits or fewer: the look-ahead table stays empty, every symbol takes the maxcode search
DC9, AC9 = flat(range(12), 9), flat(AC_SYMBOLS, 9)
# one code per length 1..16: the 16-bit one is 0xFFFE, the longest and largest a table can hold; DC16 gives it to category 11,
# AC16 (lengths 1..9 once, then 127 codes of 16 bits, 0xFF80..0xFFFE) to run 0 / size 10
DC16 = ([1] * 16, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 11])
_SHORT = [0x00, 0x01, 0xF0, 0x02, 0xF1, 0x03, 0x11, 0x04, 0x21]
AC16 = ([1] * 9 + [0] * 6 + [127], _SHORT + [s for s in AC_SYMBOLS if s not in _SHORT and s != 0x0A][:126] + [0x0A])
# 128 codes of 8 bits, the last of them 0x7F for run 14 / size 10: behind three ZRLs it codes index 63, and with the value 1023 it
# puts 17 one-bits at the end of a block
ACFF = ([0] * 7 + [128, 34] + [0] * 7, [s for s in AC_SYMBOLS if s != 0xEA][:127] + [0xEA] + [s for s in AC_SYMBOLS if s != 0xEA][127:])


def constant_blocks(values):
    """Sample values [rows, cols] (0..255) -> blocks [rows, cols, 64] that decode, with an all-ones quantisation table, to 8x8
    blocks of exactly those values: DC = 8 (v - 128), no AC."""
    v = np.asarray(values, np.int64)
    out = np.zeros(v.shape + (64,), np.int64)
    out[..., 0] = 8 * (v - 128)
    return out


def geometry(width, height, ncomp, sampling):
    """-> hs, vs, mw, mh, [block rows and columns per component]."""
    hs, vs = sampling if ncomp == 3 else (1, 1)
    mw, mh = -(-width // (8 * hs)), -(-height // (8 * vs))
    return hs, vs, mw, mh, [(mh * vs, mw * hs)] + [(mh, mw)] * (ncomp - 1)


def noise_blocks(width, height, ncomp, sampling, seed, amp=6, dc=60):
    """Seeded blocks for a picture: a DC level per block and a sprinkling of small AC coefficients."""
    rng = np.random.default_rng(seed)
    out = []
    for rows, cols in geometry(width, height, ncomp, sampling)[4]:
        b = rng.integers(-amp, amp + 1, (rows, cols, 64)) * (rng.random((rows, cols, 64)) < 0.25)
        b[..., 0] = rng.integers(-dc, dc + 1, (rows, cols))
        out.append(b.astype(np.int64))
    return out


def _segment(marker, payload, fill=0):
    return b"\xff" * (fill + 1) + bytes([marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _value_bits(v, s):
    return format(v if v > 0 else v + (1 << s) - 1, f"0{s}b") if s else ""


def _idct_range(deq):
    """Dequantised blocks [n, 64] -> (min, max) of jpeg_ref's IDCT before the level shift and the clamp."""
    x = deq.reshape(-1, 8, 8).transpose(1, 2, 0)
    out = J._idct_1d(J._idct_1d(x, 11).transpose(1, 0, 2), 18)
    return int(out.min()), int(out.max())


def write(width, height, blocks, sampling=(1, 1), *, comp_ids=(1, 2, 3), tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1), qtables=None,
          dc_tables=None, ac_tables=None, dri=None, one_segment=False, earlier=None, tables_after_sof=False, jfif=True, adobe=None,
          extra=(), fill=0, pad_bit=1, zrl_tail=False, ac_tokens=None, drop_tail_mcus=0, tail=None, fill_in_stuffing=None):
    """-> (bytes, facts).

    blocks        per component [block rows, block columns, 64]: quantised coefficients in natural order, DC absolute
    sampling      luma factors (1, 1), (2, 1) or (2, 2) of a three-component picture
    comp_ids, tq, td, ta   per component: its id, quantisation table id (0..3), DC and AC Huffman table id (0..1)
    qtables       {id: [64] natural order}; dc_tables / ac_tables {id: (counts[16], symbols)}
    dri           None: no DRI segment; an int: one; a list: one segment each, the last holds (0 or >= the MCUs: one interval)
    one_segment   every quantisation table in ONE DQT and every Huffman table in ONE DHT, else a segment per table
    earlier       {"q" / "dc" / "ac": {id: table}}: definitions written in front of the real ones, which redefine them
    tables_after_sof   DQT, DHT and DRI behind SOF0 instead of in front
    jfif, adobe   a JFIF APP0; an Adobe APP14 with this transform
    extra         [(marker, payload)] behind them (COM, APPn)
    fill          0xFF fill bytes in front of every header marker, RSTn and EOI
    pad_bit       what completes the last byte of an interval
    zrl_tail      a block whose trailing zeros are 16, 32 or 48 ends in ZRLs that land on index 64, and no EOB
    Hooks for streams that are wrong in one way (the range checks are left out when one is used):
    ac_tokens     {(component, block row, block column): [(run, size, value) | "bits"]} written in place of the block's AC part
    drop_tail_mcus     the last MCUs of the scan are not written
    tail          {interval: bytes} added behind the interval's padded last byte
    fill_in_stuffing   the n-th stuffed pair FF 00 of the scan becomes FF FF 00

    facts: intervals, ff00 (stuffed pairs), ff00_twice (two in a row), ends_ff00 (intervals whose last bytes are FF 00),
    longest_code, longest_code_value (bits of the longest code + value bits pair), idct_range, scan_bits"""
    nc = len(blocks)
    assert nc in (1, 3)
    hs, vs, mw, mh, shapes = geometry(width, height, nc, sampling)
    blocks = [np.asarray(b, np.int64).reshape(b.shape[0], b.shape[1], 64) for b in blocks]
    assert [b.shape[:2] for b in blocks] == shapes, (shapes, [b.shape for b in blocks])
    qtables = {0: ONES, 1: ONES} if qtables is None else qtables
    dc_tables = {0: DC0, 1: DC1} if dc_tables is None else dc_tables
    ac_tables = {0: AC0, 1: AC1} if ac_tables is None else ac_tables
    earlier = earlier or {}
    hooked = bool(ac_tokens or drop_tail_mcus or tail or fill_in_stuffing is not None)
    ac_tokens, tail = ac_tokens or {}, tail or {}

    # ---- the header
    q_entries = list(earlier.get("q", {}).items()) + list(qtables.items())
    h_entries = [(0, i, t) for i, t in earlier.get("dc", {}).items()] + [(1, i, t) for i, t in earlier.get("ac", {}).items()] + \
                [(0, i, t) for i, t in dc_tables.items()] + [(1, i, t) for i, t in ac_tables.items()]
    dqt = [bytes([i]) + bytes(int(np.asarray(t)[k]) for k in J.ZIGZAG) for i, t in q_entries]
    dht = [bytes([(cl << 4) | i]) + bytes(t[0]) + bytes(t[1]) for cl, i, t in h_entries]
    for _, _, t in h_entries:
        codes(t)
    dris = [] if dri is None else list(dri) if isinstance(dri, (list, tuple)) else [dri]
    tables = ([_segment(0xDB, b"".join(dqt), fill), _segment(0xC4, b"".join(dht), fill)] if one_segment else
              [_segment(0xDB, t, fill) for t in dqt] + [_segment(0xC4, t, fill) for t in dht]) + \
             [_segment(0xDD, int(r).to_bytes(2, "big"), fill) for r in dris]
    sof = _segment(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc]) +
                   b"".join(bytes([comp_ids[c], ((hs << 4) | vs) if c == 0 and nc == 3 else 0x11, tq[c]]) for c in range(nc)), fill)
    head = b"\xff\xd8"
    if jfif:
        head += _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00", fill)
    if adobe is not None:
        head += _segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([adobe]), fill)
    head += b"".join(_segment(m, p, fill) for m, p in extra)
    head += (sof + b"".join(tables)) if tables_after_sof else (b"".join(tables) + sof)
    head += _segment(0xDA, bytes([nc]) + b"".join(bytes([comp_ids[c], (td[c] << 4) | ta[c]]) for c in range(nc)) + b"\x00\x3f\x00", fill)

    # ---- the scan
    dc_codes = [codes(dc_tables[td[c]]) for c in range(nc)]
    ac_codes = [codes(ac_tables[ta[c]]) for c in range(nc)]
    facts = dict(longest_code=0, longest_code_value=0, ff00=0, ff00_twice=False, ends_ff00=[], scan_bits=0)

    def symbol(table, sym, s):
        code, length = table[sym]
        facts["longest_code"] = max(facts["longest_code"], length)
        facts["longest_code_value"] = max(facts["longest_code_value"], length + s)
        return format(code, f"0{length}b")

    def block_bits(c, by, bx, pred):
        zz = blocks[c][by, bx][J.ZIGZAG]
        diff = int(zz[0]) - pred
        s = abs(diff).bit_length()
        assert s <= 11, f"DC difference {diff}"
        out = [symbol(dc_codes[c], s, s), _value_bits(diff, s)]
        if (c, by, bx) in ac_tokens:
            for t in ac_tokens[(c, by, bx)]:
                out.append(t if isinstance(t, str) else symbol(ac_codes[c], (t[0] << 4) | t[1], t[1]) + _value_bits(t[2], t[1]))
            return "".join(out), int(zz[0])
        run = 0
        for k in range(1, 64):
            v = int(zz[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                out.append(symbol(ac_codes[c], 0xF0, 0))
                run -= 16
            s = abs(v).bit_length()
            assert s <= 10, f"AC coefficient {v}"
            out += [symbol(ac_codes[c], (run << 4) | s, s), _value_bits(v, s)]
            run = 0
        if run and zrl_tail and run % 16 == 0:
            out += [symbol(ac_codes[c], 0xF0, 0)] * (run // 16)
        elif run:
            out.append(symbol(ac_codes[c], 0x00, 0))
        return "".join(out), int(zz[0])

    n_mcu = mw * mh
    per = dris[-1] if dris and dris[-1] else n_mcu
    n_iv = -(-n_mcu // per)
    scan, stuffed = b"", 0
    for iv in range(n_iv):
        bits, pred = [], [0] * nc
        for mcu in range(iv * per, min((iv + 1) * per, n_mcu - drop_tail_mcus)):
            my, mx = divmod(mcu, mw)
            for c in range(nc):
                for k in range(hs * vs if c == 0 else 1):
                    by, bx = (my * vs + k // hs, mx * hs + k % hs) if c == 0 else (my, mx)
                    b, pred[c] = block_bits(c, by, bx, pred[c])
                    bits.append(b)
        bits = "".join(bits)
        facts["scan_bits"] += len(bits)
        bits += str(pad_bit) * (-len(bits) % 8)
        raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
        body = bytearray()
        for byte in raw:
            if byte == 0xFF:
                if fill_in_stuffing == stuffed:
                    body.append(0xFF)
                stuffed += 1
                body += b"\xff\x00"
            else:
                body.append(byte)
        body = bytes(body)
        facts["ff00"] += raw.count(0xFF)
        facts["ff00_twice"] |= b"\xff\xff" in raw
        if raw.endswith(b"\xff"):
            facts["ends_ff00"].append(iv)
        scan += body + tail.get(iv, b"")
        if iv + 1 < n_iv:
            scan += b"\xff" * (fill + 1) + bytes([0xD0 + (iv & 7)])
    facts["intervals"] = n_iv
    assert fill_in_stuffing is None or fill_in_stuffing < stuffed

    # ---- the range in which libjpeg and jpeg_ref agree by construction
    deq = np.concatenate([(blocks[c] * np.asarray(qtables[tq[c]], np.int64)).reshape(-1, 64) for c in range(nc)])
    facts["idct_range"] = _idct_range(deq)
    if not hooked:
        assert -512 <= facts["idct_range"][0] and facts["idct_range"][1] <= 511, facts["idct_range"]
    return head + scan + b"\xff" * (fill + 1) + b"\xd9", facts


# ------------------------------------------------------------------------------------------ the streams the K8 tests share
SAMPLINGS = {"gray": None, "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
QA = [1 + k % 3 for k in range(64)]
QB = [2 + (k // 8) % 2 for k in range(64)]
QC = [4 - k % 2 for k in range(64)]
RGB_IDS = (ord("R"), ord("G"), ord("B"))
# what selects tables differently from every encoder: per variant the keywords of write() for three components
SELECTIONS = {
    "all-on-1-1": dict(td=(1, 1, 1), ta=(1, 1, 1), tq=(1, 1, 1), qtables={1: QB}, dc_tables={1: DC1}, ac_tables={1: AC1}),
    "luma-1-0-chroma-0-1": dict(td=(1, 0, 0), ta=(0, 1, 1), qtables={0: QA, 1: QB}),
    "cb-0-1-cr-1-0": dict(td=(0, 0, 1), ta=(0, 1, 0), qtables={0: QA, 1: QB}),
    "q-2-3-1": dict(tq=(2, 3, 1), qtables={1: QA, 2: QB, 3: QC}),
    "redefined": dict(tq=(0, 1, 1), qtables={0: QA, 1: QB}, earlier={"q": {0: QC, 1: QA}, "dc": {0: DC1, 1: DC9}, "ac": {0: AC9, 1: AC0}}),
    "one-segment": dict(tq=(0, 1, 2), qtables={0: QA, 1: QB, 2: QC}, td=(0, 1, 0), ta=(1, 0, 1), one_segment=True),
    "after-sof": dict(tq=(0, 1, 0), qtables={0: QB, 1: QC}, td=(1, 0, 1), tables_after_sof=True),
}
COMMENT = b"a comment with \xff\xd8 and \xff\xda and \xff\xd9 and \xff\x00 inside"
# how the marker segments can lie (a 40x24 4:2:0 picture: 3 x 2 MCUs) -> (keywords, restart interval, intervals)
LAYOUTS = {
    "plain": (dict(), 0, 1),
    "no-jfif": (dict(jfif=False), 0, 1),
    "adobe-1": (dict(jfif=False, adobe=1), 0, 1),
    "jfif-and-adobe-1": (dict(adobe=1), 0, 1),
    "com-and-app": (dict(extra=[(0xFE, COMMENT), (0xE1, b"Exif\x00\x00" + COMMENT), (0xED, COMMENT * 3)]), 0, 1),
    "fill-bytes": (dict(fill=3, dri=2), 2, 3),
    "one-segment-after-sof": (dict(one_segment=True, tables_after_sof=True, dri=4), 4, 2),
    "dri-1": (dict(dri=1), 1, 6),
    "dri-above-mcus": (dict(dri=7), 7, 1),
    "dri-equals-mcus": (dict(dri=6), 6, 1),
    "dri-0": (dict(dri=0), 0, 1),
    "dri-twice": (dict(dri=[1, 3]), 3, 2),
    "dri-then-0": (dict(dri=[2, 0]), 0, 1),
    "ids-0-1-2": (dict(jfif=False, comp_ids=(0, 1, 2)), 0, 1),
    "ids-7-33-200": (dict(jfif=False, comp_ids=(7, 33, 200)), 0, 1),
    "rgb-ids-with-jfif": (dict(comp_ids=RGB_IDS), 0, 1),
    "rgb-ids-with-adobe-1": (dict(jfif=False, adobe=1, comp_ids=RGB_IDS), 0, 1),
}


def _zz(pairs):
    """{zigzag index: value} -> one block [64] in natural order."""
    b = np.zeros(64, np.int64)
    for k, v in pairs.items():
        b[J.ZIGZAG[k]] = v
    return b


def edge_blocks():
    """A gray 40x16 picture (5 x 2 blocks) of block shapes no encoder writes, from the symbols AC16 has: DC differences of +2047
    and -2047 (category 11) in front of +-1023 (run 0 / size 10); 47, 31 and 15 coefficients and then zeros up to index 63 (with
    zrl_tail: ZRLs that land exactly on 64); a run of 15 in front of a coefficient, alone and behind a ZRL; 63 non-zero ACs
    and no EOB; an immediate EOB; a few ordinary run / size pairs."""
    sign = lambda k: 1 if k % 3 else -1
    shapes = [{0: 2047, 1: 1023}, {0: 0, 1: -1023},
              {0: 40, **{k: sign(k) for k in range(1, 48)}}, {0: -40, **{k: -sign(k) for k in range(1, 32)}}, {0: 8, **{k: sign(k) for k in range(1, 16)}},
              {0: -300, 16: 1}, {0: 300, 33: -1, 49: 1}, {0: 0, **{k: sign(k) for k in range(1, 64)}}, {0: 100},
              {0: -100, 1: 5, 2: -9, 4: 1, 7: -1, 8: 3}]
    return [np.stack([_zz(s) for s in shapes]).reshape(2, 5, 64)]


def ff_blocks(cols, rows):
    """Gray blocks whose last coefficient, index 63 behind three ZRLs and run 14, is 1023: with ACFF every block ends in 17
    one-bits, so every interval ends in two stuffed bytes and others lie inside."""
    out = np.zeros((rows, cols, 64), np.int64)
    for i in range(rows * cols):
        out[i // cols, i % cols] = _zz({0: (i * 37) % 200 - 100, 1: (i % 5) - 2, 63: 1023})
    return [out]


_cache = {}


def _memo(fn):
    def wrapped():
        if fn.__name__ not in _cache:
            _cache[fn.__name__] = fn()
        return _cache[fn.__name__]
    return wrapped


@_memo
def selection_streams():
    """{name: (bytes, facts)}: 16x16 and 24x16 pictures, gray and the three samplings, every variant of SELECTIONS."""
    out = {}
    for w, h in [(16, 16), (24, 16)]:
        for sname, sampling in SAMPLINGS.items():
            nc = 1 if sampling is None else 3
            for vname, kw in SELECTIONS.items():
                blocks = noise_blocks(w, h, nc, sampling, seed=w + len(out))
                out[f"{w}x{h}-{sname}-{vname}"] = write(w, h, blocks, sampling or (1, 1), dri=[0, 1, 2][len(out) % 3] or None, **kw)
    return out


@_memo
def layout_streams():
    return {name: write(40, 24, noise_blocks(40, 24, 3, (2, 2), seed=3), (2, 2), qtables={0: QA, 1: QB}, **kw) for name, (kw, _, _) in LAYOUTS.items()}


def rgb_ids_stream():
    return write(40, 24, noise_blocks(40, 24, 3, (1, 1), seed=4), (1, 1), comp_ids=RGB_IDS, jfif=False)[0]


@_memo
def entropy_streams():
    out = {}
    for tname, (dc, ac) in {"annex-k": (DC0, AC0), "nine-bit": (DC9, AC9), "sixteen-bit": (DC16, AC16)}.items():
        for dri in (None, 3):
            out[f"edges-{tname}-dri-{dri}"] = write(40, 16, edge_blocks(), td=(0,), ta=(0,), tq=(0,), dc_tables={0: dc}, ac_tables={0: ac}, dri=dri,
                                                    zrl_tail=True)
    ff = dict(td=(0,), ta=(0,), tq=(0,), ac_tables={0: ACFF}, dri=2)
    out["stuffed"] = write(64, 32, ff_blocks(8, 4), **ff)
    out["stuffed-fill"] = write(64, 32, ff_blocks(8, 4), fill=2, **ff)
    out["stuffed-pad-0"] = write(64, 32, ff_blocks(8, 4), pad_bit=0, **ff)
    out["nine-bit-4:2:0"] = write(24, 16, noise_blocks(24, 16, 3, (2, 2), seed=9), (2, 2), dc_tables={0: DC9, 1: DC0}, ac_tables={0: AC9, 1: AC9},
                                  qtables={0: QA, 1: QB}, pad_bit=0, fill=1, dri=1)
    return out


@_memo
def lane_streams():
    """More restart intervals than one block of 64 entropy lanes, beside pictures of one interval."""
    return {"72-intervals-4:4:4": write(72, 64, noise_blocks(72, 64, 3, (1, 1), seed=5), (1, 1), dri=1, qtables={0: QA, 1: QB}),
            "40-intervals-4:2:0": write(128, 72, noise_blocks(128, 72, 3, (2, 2), seed=6), (2, 2), dri=1, qtables={0: QA, 1: QB}),
            "one-interval": write(40, 24, noise_blocks(40, 24, 3, (2, 1), seed=7), (2, 1)),
            "gray": write(24, 40, noise_blocks(24, 40, 1, None, seed=8), dri=2)}


@_memo
def range_streams():
    """constant_blocks pictures in which every Y, Cb and Cr value 0..255 occurs (256 chroma blocks each), for the NV12 range ends."""
    v = np.arange(256)
    out = {}
    for name, (hs, vs) in {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}.items():
        y = np.repeat(np.repeat(v.reshape(16, 16), vs, 0), hs, 1)
        y = (y + (np.arange(y.shape[0])[:, None] % vs) * 128 + (np.arange(y.shape[1])[None, :] % hs) * 64) % 256
        blocks = [constant_blocks(y), constant_blocks(((v * 7 + 3) % 256).reshape(16, 16)), constant_blocks(((255 - v) * 11 % 256).reshape(16, 16))]
        out[f"range-{name}"] = write(128 * hs, 128 * vs, blocks, (hs, vs), dri=16)
    return out


CHROMA16 = [0, 255, 1, 254, 16, 240, 64, 192, 100, 128, 127, 129, 90, 171, 35, 220]


@_memo
def bgr_range_stream():
    """4:4:4, 256x192: Y in {0, 128, 255} x Cb x Cr over CHROMA16 -- every corner of jdcolor.c's conversion and its clamps."""
    y = np.repeat(np.array([0, 128, 255]), 256).reshape(24, 32)
    cb = np.tile(np.repeat(np.array(CHROMA16), 16), 3).reshape(24, 32)
    cr = np.tile(np.array(CHROMA16), 48).reshape(24, 32)
    return write(256, 192, [constant_blocks(y), constant_blocks(cb), constant_blocks(cr)], (1, 1), dri=32)


def good_streams():
    """Every well-formed YCbCr or gray stream of the K8 tests: {name: (bytes, facts)}."""
    out = {}
    for part in (selection_streams(), layout_streams(), entropy_streams(), lane_streams(), range_streams(), {"bgr-range": bgr_range_stream()}):
        out.update(part)
    return out


@_memo
def bad_streams():
    """{name: (bytes, facts)}: gray 32x16 pictures (4 x 2 blocks, Annex K's code lengths) that the parser accepts and that are
    wrong in exactly one of the ways k8_entropy documents, and well-formed otherwise."""
    blocks = noise_blocks(32, 16, 1, None, seed=11)
    base = dict(td=(0,), ta=(0,), tq=(0,))
    dense = lambda n: [(0, 1, 1 if k % 2 else -1) for k in range(n)]
    return {
        # sixteen one-bits where an AC code is due: AC0's largest 16-bit code is below 0xFFFF
        "code-in-no-table": write(32, 16, blocks, ac_tokens={(0, 0, 2): ["1" * 16]}, **base),
        # 60 coefficients (index 60 is done), then run 5: index 66
        "run-past-63": write(32, 16, blocks, ac_tokens={(0, 1, 1): dense(60) + [(5, 1, 1), (0, 0, 0)]}, **base),
        # 62 coefficients (index 62 is done), then a ZRL: index 79
        "zrl-past-64": write(32, 16, blocks, ac_tokens={(0, 0, 3): dense(62) + [(15, 0, 0)]}, **base),
        # the last four blocks are missing: the zero bits past the end read as DC category 0 + EOB (codes 00, 00), so the lane ends
        # in order, 16 bits short
        "interval-runs-dry": write(32, 16, blocks, drop_tail_mcus=4, pad_bit=0, **base),
        "bytes-left-over": write(32, 16, blocks, tail={0: b"\x55\xaa"}, **base),
        "ff-ff-00": write(48, 32, ff_blocks(6, 4), td=(0,), ta=(0,), tq=(0,), ac_tables={0: ACFF}, dri=2, fill_in_stuffing=5),
        "extra-00-before-eoi": write(32, 16, blocks, tail={0: b"\x00"}, **base),
    }
