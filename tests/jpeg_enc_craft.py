"""Images crafted in the coefficient domain for K7, the device JPEG encoder (csrc/rva_jpeg.hip), and an analyser that says what an
image makes the entropy coder do.  ``synth.make_bgr`` gives smooth pictures: a fraction of the Annex-K symbols, no DC step of
category 11, whatever 0xFF bytes happen.  The generators here aim at the rest -- every (run, size) symbol of both AC tables, ZRL
chains, blocks without EOB, every DC category in both signs across MCUs, restarts and dummy blocks, the longest blocks an image can
give, 0xFF bytes at the edges of the kernel's 64-byte stuffing steps and 64-block passes -- and ``facts`` measures, through
``oracle/jpeg_oracle.py`` alone, which of them an image reaches.  tests/test_jpeg_enc_craft_host.py asserts the coverage of the whole
set and pins the oracle to Pillow's libjpeg on it; tests/test_gpu_jpeg_enc_craft.py holds K7 to the oracle's bytes on it.

Everything is deterministic.  A generator returns ``(uint8 [h, w, 3] BGR, quality)``; no image is larger than 512 x 160."""
import functools

import numpy as np

from oracle import jpeg_oracle as J

MAX_W, MAX_H = 512, 160
_A = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
# zigzag positions of the first row / column of a block (one cosine: amplitude F / 5.66 instead of F / 4, so the largest coefficients)
_EDGE = [35, 28, 27, 21, 20, 15, 14, 10, 9, 6, 5, 3, 2, 1]


# ------------------------------------------------------------------------------------------ symbol sheets
def _targets():
    """[(anchor position or 0, anchor value, position, size, sign)]: single coefficients at every zigzag position 1..63 (run 0..62,
    i.e. up to three ZRLs, and position 63 leaves no EOB), then a +-1 anchor 0..15 zeros before a coefficient (any run before any
    size), each for size 1..10 in both signs; one flat block (EOB only) first."""
    out = [(0, 0, 0, 0, 0)]
    for size in range(1, 11):
        for pos in range(1, 64):
            for sign in (1, -1):
                out.append((0, 0, pos, size, sign))
    for size in range(1, 11):
        for run in range(16):
            for sign in (1, -1):
                for pos in [p for p in _EDGE + [63] if p - run - 1 >= 1][:3]:      # three positions: what one misses another may reach
                    out.append((pos - run - 1, -sign, pos, size, sign))
    return out


def _magnitudes(size):
    """Values of one size (category) to try, the widest first: both ends of the category are wanted, most of all the upper."""
    lo, hi = 1 << (size - 1), (1 << size) - 1
    return sorted({hi, lo, *range(hi, lo, -max(1, (hi - lo) // 24))}, reverse=True)


def _pick(qtbl, lo, hi):
    """The 8x8 sample blocks (int, lo..hi) of the targets: per target the first magnitude of its size whose samples stay in range
    and whose quantised coefficients -- by the oracle's own DCT and quantiser -- have the wanted size and sign at the position and
    only zeros between it and the anchor (or the DC).  A target without such a magnitude is left out: at quality 100 every table
    entry is 1 and half a grey level of rounding can surface as a stray +-1 inside the run.  Of the anchored targets one position
    per (run, size, sign) is kept."""
    targets = _targets()
    cand, owner = [], []
    for ti, (apos, aval, pos, size, sign) in enumerate(targets):
        mags = _magnitudes(size) if size else [0]
        for m in mags:
            f = np.zeros(64)
            if size:
                f[J.ZIGZAG[pos]] = sign * m * qtbl[J.ZIGZAG[pos]]
            if apos:
                f[J.ZIGZAG[apos]] = aval * qtbl[J.ZIGZAG[apos]]
            cand.append(f)
            owner.append((ti, sign * m))
    f = np.array(cand).reshape(-1, 8, 8)
    pix = np.rint(_A.T @ f @ _A + 128.0).astype(np.int64)
    inside = (pix.min(axis=(1, 2)) >= lo) & (pix.max(axis=(1, 2)) <= hi)
    got = J.quantise(J.fdct_islow(pix - 128), qtbl).reshape(-1, 64)[:, J.ZIGZAG]
    blocks, anchored = [None] * len(targets), set()
    for i, (ti, val) in enumerate(owner):
        apos, aval, pos, size, sign = targets[ti]
        if blocks[ti] is not None or not inside[i] or (apos and (pos - apos, size, sign) in anchored):      # one position per anchored symbol
            continue
        g = got[i]
        # the symbol is decided by the coefficient and the zeros before it; a stray +-1 BEHIND it only adds a symbol of its own
        if g[pos] * val >= 0 and abs(int(g[pos])).bit_length() == size and not g[apos + 1:pos].any() and (apos == 0 or g[apos] != 0):
            blocks[ti] = pix[i]
            if apos:
                anchored.add((pos - apos, size, sign))
    return [b for b in blocks if b is not None]


@functools.lru_cache(maxsize=None)
def _chroma_lut(plane):
    """value t of the Cb (plane 1) or Cr (plane 2) sample -> (B, G, R) that the oracle's colour conversion maps to exactly t in
    that plane and exactly 128 in the other.  Y = 128 where the gamut allows (B = 128 + 1.772 d, G = 128 - 0.344 d, R = 128 for
    Cb: |d| <= 71); beyond that the nearest luma that keeps the colour inside the cube, which reaches |d| = 120."""
    lut = {}
    for t in range(256):
        d = t - 128
        for y in sorted(range(256), key=lambda v: abs(v - 128)):
            if plane == 1:
                rgb = (y, y - 0.344136 * d, y + 1.772 * d)
            else:
                rgb = (y + 1.402 * d, y - 0.714136 * d, y)
            if min(rgb) < -0.5 or max(rgb) > 255.5:
                continue
            base = [int(round(v)) for v in rgb]
            hit = None
            for dr in (0, -1, 1):
                for dg in (0, -1, 1):
                    for db in (0, -1, 1):
                        r, g, b = base[0] + dr, base[1] + dg, base[2] + db
                        if min(r, g, b) < 0 or max(r, g, b) > 255:
                            continue
                        cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
                        cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
                        if (cb, cr) == ((t, 128) if plane == 1 else (128, t)) and hit is None:
                            hit = (b, g, r)
            if hit:
                lut[t] = hit
                break
    return lut


@functools.lru_cache(maxsize=None)
def _sheet_blocks(kind, q):
    ql, qc = J.quant_tables(q)
    if kind == "luma":
        return _pick(ql, 0, 255)
    lut = _chroma_lut(1)
    lo = min(set(lut) & set(_chroma_lut(2)))
    hi = max(set(lut) & set(_chroma_lut(2)))
    assert all(t in lut and t in _chroma_lut(2) for t in range(lo, hi + 1))
    return _pick(qc, lo, hi)


def sheet_parts(kind, q):
    """How many images ``symbol_sheet(kind, q, part)`` splits its blocks into (an image holds 64 x 20 luma or 32 x 10 chroma blocks)."""
    per = (MAX_W // 8) * (MAX_H // 8) if kind == "luma" else (MAX_W // 16) * (MAX_H // 16)
    return -(-len(_sheet_blocks(kind, q)) // per)


def symbol_sheet(kind, q, part=0):
    """One 8x8 block per AC pattern (see ``_targets``), each the inverse DCT of one or two quantised coefficients times the table
    of quality ``q``, rounded to samples; patterns whose samples leave the range, or whose rounding puts a stray coefficient into the
    run of zeros, are left out (``_pick``).  "luma": grey blocks 8 px apart (chroma flat).  "chroma": the same patterns as 8x8 CHROMA blocks, every sample
    a 2x2 square of pixels, MCUs alternating between the Cb and the Cr plane (even / odd; ``part`` odd swaps them).  Rows of at
    most 512 px; what one image of 160 rows does not hold goes to the next ``part``."""
    blocks = _sheet_blocks(kind, q)
    cell = 8 if kind == "luma" else 16
    per = (MAX_W // cell) * (MAX_H // cell)
    mine = blocks[part * per:(part + 1) * per]
    assert mine, (kind, q, part)
    cols = min(len(mine), MAX_W // cell)
    rows = -(-len(mine) // cols)
    img = np.full((rows * cell, cols * cell, 3), 128, np.uint8)
    for i, blk in enumerate(mine):
        y, x = i // cols * cell, i % cols * cell
        if kind == "luma":
            img[y:y + 8, x:x + 8, :] = blk[:, :, None]
        else:
            lut = _chroma_lut(1 + (i + part) % 2)
            img[y:y + 16, x:x + 16, :] = np.array([[lut[int(v)] for v in row] for row in blk], np.uint8).repeat(2, 0).repeat(2, 1)
    return img, q


# ------------------------------------------------------------------------------------------ DC steps
BLUE, YELLOW, RED, CYAN = (255, 0, 0), (0, 255, 255), (0, 0, 255), (255, 255, 0)        # BGR


def _dc_magnitudes():
    return [m for c in range(1, 12) for m in sorted({1 << (c - 1), min((1 << c) - 1, 2040)})]


def _grey_tile(dc):
    """An 8x8 grey tile whose quantised luma DC at quality 100 is ``dc`` (-1024..1016): flat at 128 + dc // 8, and for the
    categories below 4, which a flat tile cannot step by (its DC is a multiple of 8), ``dc % 8`` rows one level brighter."""
    v, k = 128 + dc // 8, dc % 8
    t = np.full((8, 8, 3), v, np.uint8)
    t[:k] += 1
    return t


def _axis_colour(plane, dc):
    """A colour whose Cb (plane 1) or Cr (plane 2) DC at quality 100 is 8 * (dc // 8) and whose other chroma plane is 128; the
    ends of the axes are the saturated blue / yellow and red / cyan."""
    t = 128 + dc // 8
    lut = _chroma_lut(plane)
    if t in lut:
        return lut[t]
    if plane == 1:
        return BLUE if t > 128 else YELLOW
    return RED if t > 128 else CYAN


def dc_steps():
    """16x16 MCUs of flat 8x8 tiles at quality 100 whose DC differences, in MCU coding order, take every category 0..11 in both
    signs: MCU row 0 greys (black, white and between: 2040 = black -> white is category 11), rows 1 and 2 colours along blue --
    yellow (Cb: +-2040), rows 3 and 4 along red -- cyan (Cr).  Chroma has one sample per 2x2 pixels, so a chroma tile is 16x16 and its DC a multiple
    of 8; the categories 1..3 of Cb / Cr come from tiles split into two colours one level apart.  Every row starts with a blue MCU and
    ends with a yellow one: Y, Cb and Cr of the first block of a row differ from the last block of the row before by 1576, 2040 and
    336 (categories 11, 11, 9), so a predictor that survived the restart marker would change the bytes."""
    mags = _dc_magnitudes()
    # row 0: luma walks from black up by m and back down, four tiles per MCU
    dcs = [-1024, -1024]
    for m in mags:
        dcs += [-1024 + m, -1024]
    dcs += [dcs[-1]] * (-len(dcs) % 4)
    tiles = [_grey_tile(d) for d in dcs]
    luma_row = []
    for i in range(0, len(tiles), 4):
        m = np.empty((16, 16, 3), np.uint8)
        m[:8, :8], m[:8, 8:], m[8:, :8], m[8:, 8:] = tiles[i:i + 4]
        luma_row.append(m)
    rows = [luma_row]
    for plane in (1, 2):
        row = []
        for m in [0] + mags:
            lo = -1024 if m > 1023 else -896                         # the saturated end only where the step needs it
            for dc in (lo + m, lo):
                mcu = np.empty((16, 16, 3), np.uint8)
                mcu[:] = _axis_colour(plane, dc)
                k = dc % 8                                           # 2k of 16 pixel rows one chroma level up: + k in the DC
                if k:
                    mcu[:2 * k] = _axis_colour(plane, dc + 8)
                row.append(mcu)
        rows += [row[:len(row) // 2], row[len(row) // 2:]]           # two MCU rows per plane: 512 px hold 32 MCUs
    n = max(len(r) for r in rows) + 2
    assert n * 16 <= MAX_W
    img = np.full((len(rows) * 16, n * 16, 3), 128, np.uint8)
    for y, row in enumerate(rows):
        img[y * 16:(y + 1) * 16, :16] = BLUE
        img[y * 16:(y + 1) * 16, -16:] = YELLOW
        for x, mcu in enumerate(row):
            img[y * 16:(y + 1) * 16, (x + 1) * 16:(x + 2) * 16] = mcu
    return img, 100


def dc_edge(w, h):
    """Black and white 8x8 tiles on a 3x3 grid, cropped to ``w`` x ``h`` (24x24, 8x24, 24x8) at quality 100: images that end half
    way through an MCU, so libjpeg pads with dummy luma blocks that copy the DC before them -- and in each the block coded after a
    dummy one differs from it by 2040, category 11 (a dummy block that copied the wrong DC moves the bytes the most)."""
    grid = np.array([[255, 0, 255], [0, 255, 0], [0, 255, 0]], np.uint8)
    img = grid.repeat(8, 0).repeat(8, 1)[:h, :w, None].repeat(3, 2)
    return np.ascontiguousarray(img), 100


# ------------------------------------------------------------------------------------------ noise
def dense_noise(seed, w, h):
    """0 or 255 per channel and pixel at quality 100: the longest coded blocks an image can give, and 0xFF bytes everywhere."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 255], np.uint8), size=(h, w, 3)), 100


def noise(seed, w, h, q):
    """``dense_noise`` at any quality (lower qualities code shorter blocks: other phases of the 64-byte steps and 64-block passes)."""
    return dense_noise(seed, w, h)[0], q


# (seed, w, h, q) of ``noise`` images found by a search on the CPU (tests/test_jpeg_enc_craft_host.py asserts, through ``facts``,
# that together they show every entry of STUFFING_FACTS); 176 px and wider, so an interval has more than 64 blocks and a second pass
PINNED = [(82, 192, 16, 100), (185, 192, 16, 100), (5068, 176, 160, 97)]


def pinned_stuffing_cases():
    return list(PINNED)


# ------------------------------------------------------------------------------------------ the analyser
STUFFING_FACTS = ("ff_at_lane_0", "ff_at_lane_63", "four_ff_in_a_step", "ff_ff_adjacent", "ff_last_byte_of_a_nonfinal_pass",
                  "ff_first_byte_of_a_pass_with_carry", "interval_ends_byte_aligned", "pad_byte_is_ff")
PASS_BLOCKS, STEP_BYTES = 64, 64            # k7_entropy: blocks per pass, bytes per stuffing step


class _Recorder:
    """What ``_encode_block`` writes, as bits, without stuffing."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, size):
        self.acc = (self.acc << size) | (code & ((1 << size) - 1))
        self.n += size


def _interval_facts(rec, ends, out):
    """The interval's bits split as k7_entropy splits them: a pass is 64 blocks, its bytes are the complete ones of carry + bits,
    a stuffing step is 64 of those bytes."""
    total = rec.n
    data = (rec.acc << (-total % 8)).to_bytes((total + 7) // 8, "big") if total else b""
    found = set()
    bounds = [ends[i] for i in range(PASS_BLOCKS - 1, len(ends), PASS_BLOCKS)]
    if not bounds or bounds[-1] != total:
        bounds.append(total)
    start_bits = 0
    for pi, end_bits in enumerate(bounds):
        first, last = start_bits >> 3, end_bits >> 3                  # this pass stuffs bytes [first, last)
        chunk = data[first:last]
        for s in range(0, len(chunk), STEP_BYTES):
            step = chunk[s:s + STEP_BYTES]
            if step[0] == 0xFF:
                found.add("ff_at_lane_0")
            if len(step) == STEP_BYTES and step[-1] == 0xFF:
                found.add("ff_at_lane_63")
            if step.count(0xFF) >= 4:
                found.add("four_ff_in_a_step")
            if b"\xff\xff" in step:
                found.add("ff_ff_adjacent")
        if chunk and pi + 1 < len(bounds) and chunk[-1] == 0xFF:
            found.add("ff_last_byte_of_a_nonfinal_pass")
        if chunk and start_bits & 7 and chunk[0] == 0xFF:
            found.add("ff_first_byte_of_a_pass_with_carry")
        start_bits = end_bits
    if total % 8 == 0:
        found.add("interval_ends_byte_aligned")
    elif (data[-1] | (0xFF >> (total % 8))) == 0xFF:
        found.add("pad_byte_is_ff")
    for f in found:
        out[f] += 1


def facts(bgr, q):
    """What encoding ``bgr`` at quality ``q`` exercises, from the oracle's coefficients, code tables and block coder alone:
    ``ac`` {table: {(run, size)}}, ``zrl`` {table: {ZRLs in a row}}, ``dc`` {component: {(category, sign)}}, ``no_eob`` /
    ``eob_only`` {table: blocks}, ``max_block_bits``, ``stuffing`` {fact: intervals that show it}."""
    (cy, ccb, ccr), _ = J.coefficients(bgr, q)
    mh, mw = cy.shape[0] // 2, cy.shape[1] // 2
    tabs = {"luma": (J.huff_codes(*J.DC_LUMA), J.huff_codes(*J.AC_LUMA)), "chroma": (J.huff_codes(*J.DC_CHROMA), J.huff_codes(*J.AC_CHROMA))}
    out = {"ac": {"luma": set(), "chroma": set()}, "zrl": {"luma": set(), "chroma": set()}, "dc": {"y": set(), "cb": set(), "cr": set()},
           "no_eob": {"luma": 0, "chroma": 0}, "eob_only": {"luma": 0, "chroma": 0}, "max_block_bits": 0,
           "stuffing": {f: 0 for f in STUFFING_FACTS}, "intervals": mh, "passes_per_interval": -(-mw * 6 // PASS_BLOCKS)}
    for my in range(mh):
        rec, ends = _Recorder(), []
        pred = {"y": 0, "cb": 0, "cr": 0}
        for mx in range(mw):
            blocks = [("y", "luma", cy[2 * my + by, 2 * mx + bx]) for by, bx in ((0, 0), (0, 1), (1, 0), (1, 1))]
            blocks += [("cb", "chroma", ccb[my, mx]), ("cr", "chroma", ccr[my, mx])]
            for comp, tab, zz in blocks:
                diff = int(zz[0]) - pred[comp]
                out["dc"][comp].add((abs(diff).bit_length(), (diff > 0) - (diff < 0)))
                nz = np.flatnonzero(zz[1:]) + 1
                prev = 0
                for k in nz:
                    run = int(k) - prev - 1
                    if run > 15:
                        out["zrl"][tab].add(run // 16)
                    out["ac"][tab].add((run % 16, abs(int(zz[k])).bit_length()))
                    prev = int(k)
                out["no_eob"][tab] += int(zz[63] != 0)
                out["eob_only"][tab] += int(len(nz) == 0)
                before = rec.n
                pred[comp] = J._encode_block(rec, zz, pred[comp], *tabs[tab])
                out["max_block_bits"] = max(out["max_block_bits"], rec.n - before)
                ends.append(rec.n)
        _interval_facts(rec, ends, out["stuffing"])
    return out


# ------------------------------------------------------------------------------------------ the set
SHEETS = (("luma", 100), ("luma", 90), ("chroma", 100), ("chroma", 75))
# the names ``crafted`` gives, spelled out so that a test can be parametrised without building the images at collection time
NAMES = ("sheet-luma-q100-0", "sheet-luma-q90-0", "sheet-chroma-q100-0", "sheet-chroma-q100-1", "sheet-chroma-q100-2",
         "sheet-chroma-q75-0", "sheet-chroma-q75-1", "sheet-chroma-q75-2", "dc-steps", "dc-edge-24x24", "dc-edge-8x24", "dc-edge-24x8",
         "dense-0-16x16", "dense-1-192x16", "dense-2-200x40", "pinned-82-192x16-q100", "pinned-185-192x16-q100",
         "pinned-5068-176x160-q97")


@functools.lru_cache(maxsize=None)
def crafted():
    """{name: (image, quality)} of the whole crafted set, built once; the images are read-only."""
    out = {}
    for kind, q in SHEETS:
        for part in range(sheet_parts(kind, q)):
            out[f"sheet-{kind}-q{q}-{part}"] = symbol_sheet(kind, q, part)
    out["dc-steps"] = dc_steps()
    for w, h in ((24, 24), (8, 24), (24, 8)):
        out[f"dc-edge-{w}x{h}"] = dc_edge(w, h)
    for seed, w, h in ((0, 16, 16), (1, 192, 16), (2, 200, 40)):
        out[f"dense-{seed}-{w}x{h}"] = dense_noise(seed, w, h)
    for seed, w, h, q in pinned_stuffing_cases():
        out[f"pinned-{seed}-{w}x{h}-q{q}"] = noise(seed, w, h, q)
    for img, _ in out.values():
        assert img.dtype == np.uint8 and img.shape[2] == 3 and img.shape[0] <= MAX_H and img.shape[1] <= MAX_W
        img.setflags(write=False)
    return out


def coverage(found=None):
    """The set's measured coverage as plain data (profiles/jpeg_enc_craft.json): per image its geometry and largest block, then
    over the set the AC symbols per table, ZRL chains, block ends, DC categories per component and which image shows each
    stuffing fact.  ``found``: {name: facts} when the caller has them already."""
    found = found or {name: facts(img, q) for name, (img, q) in crafted().items()}
    every = [(run, size) for run in range(16) for size in range(1, 11)]
    rep = {"images": {}, "ac_symbols": {}, "zrl_chains": {}, "blocks_without_eob": {}, "blocks_of_eob_only": {}, "dc_categories": {},
           "stuffing": {}}
    for name, f in found.items():
        img, q = crafted()[name]
        rep["images"][name] = {"width": img.shape[1], "height": img.shape[0], "quality": q, "intervals": f["intervals"],
                               "passes_per_interval": f["passes_per_interval"], "max_block_bits": f["max_block_bits"]}
    for tab in ("luma", "chroma"):
        got = set().union(*(f["ac"][tab] for f in found.values()))
        rep["ac_symbols"][tab] = {"coded": len(got & set(every)), "of": len(every), "missing": [list(s) for s in every if s not in got]}
        rep["zrl_chains"][tab] = sorted(set().union(*(f["zrl"][tab] for f in found.values())))
        rep["blocks_without_eob"][tab] = sum(f["no_eob"][tab] for f in found.values())
        rep["blocks_of_eob_only"][tab] = sum(f["eob_only"][tab] for f in found.values())
    for comp in ("y", "cb", "cr"):
        rep["dc_categories"][comp] = sorted(c * s for c, s in set().union(*(f["dc"][comp] for f in found.values())))
    for fact in STUFFING_FACTS:
        rep["stuffing"][fact] = {name: f["stuffing"][fact] for name, f in found.items() if f["stuffing"][fact] and name.startswith("pinned-")}
    top = max(found, key=lambda n: found[n]["max_block_bits"])
    rep["max_block_bits"] = {"bits": found[top]["max_block_bits"], "image": top, "dense-0-16x16": found["dense-0-16x16"]["max_block_bits"],
                             "k7_private_buffer_bits": 1728}
    return rep
