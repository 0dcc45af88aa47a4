"""The JPEG decoder's cases and its host model (numpy / Python; no test in here).  The model restates the format of
include/ppst_hip.h "JPEG decode on the device" stage by stage -- the clean stream, the SUBSEQUENCE ITERATION itself (not a
sequential decode), the block prefix and write pass, DC prediction, libjpeg's integer IDCT, fancy upsampling and colour -- from a
descriptor (the fields ppst_jpeg_parse fills) and the file's bytes.  It never calls a kernel.  Every array it indexes is a
``Checked`` list: an index below 0 or beyond the end raises, so a damaged file that finishes here has stayed inside every array.

The judge of the pixels is Pillow (jpeg_cases.pillow_decode); the judge of the coefficients is jpeg_cases.entropy_decode."""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as J  # noqa: E402

SUBSEQ_DEFAULT = 32                    # words (JD_SUBSEQ_DEFAULT of csrc/jpeg_decode.hip)
S_MARKER, S_RST_COUNT, S_RST_ORDER, S_CODE, S_BLOCKS = 1, 2, 4, 8, 16        # PPST_JPEG_S_*
SMALL = ("1x1", "8x8", "16x16", "1x1_grey", "17x3", "41x77", "checker1", "checker8", "random96", "random96_grey", "smooth",
         "photo96x136", "photo41x77")                                          # up to 96 x 136: the full cross-product
LARGE = ("160x136", "200x232", "8x2100", "2100x8", "64x700_grey", "zeros", "ones")     # one setting each on the CPU


class Checked(list):
    """a list whose indices must be 0 .. len - 1 (a plain list takes negative ones)"""

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError("read at %d of %d" % (i, len(self)))
        return list.__getitem__(self, i)

    def __setitem__(self, i, v):
        if not 0 <= i < len(self):
            raise IndexError("write at %d of %d" % (i, len(self)))
        list.__setitem__(self, i, v)


# ------------------------------------------------------------------------------------------------------------------- files
def pillow_file(arr, quality, subsampling, optimize=False, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(buf, format="JPEG", quality=quality, subsampling=J.SS_NUMBER[subsampling],
                                                                    optimize=optimize, **kw)
    return buf.getvalue()


def damaged_files(blob, flips=200, seed=11):
    """every prefix of the file, then `flips` copies with one byte of the scan replaced (seeded positions and values)"""
    p = J.parse(blob)
    out = [blob[:n] for n in range(len(blob))]
    rng = np.random.default_rng(seed)
    lo, hi = len(p["head"]), len(blob) - 2
    for at, v in zip(rng.integers(lo, hi, flips).tolist(), rng.integers(1, 256, flips).tolist()):
        out.append(blob[:at] + bytes([blob[at] ^ v]) + blob[at + 1:])
    return out


def damage_source():
    """the small file the truncation / corruption lists are made of: DRI, both chroma planes, a few hundred bytes of scan"""
    return J.model_encode(J.image_set()["41x77"], 50, "4:2:0", R=4)


def dump_damaged(directory):
    """the same files as damaged_files(damage_source()), one per file, for tests/jpeg_parse_san.cpp"""
    os.makedirs(directory, exist_ok=True)
    for n, b in enumerate(damaged_files(damage_source())):
        with open(os.path.join(directory, "%05d.jpg" % n), "wb") as f:
            f.write(b)


# ------------------------------------------------------------------------------------------------------------- descriptor
class Desc:
    """the descriptor's fields as plain Python (from the ctypes structure ppst_jpeg_parse filled)"""

    def __init__(self, d):
        self.H, self.W, self.ncomp, self.ss, self.dri = d.H, d.W, d.ncomp, d.ss, d.dri
        self.scan_off, self.scan_len = d.scan_off, d.scan_len
        self.qt = [[d.qt[c][k] for k in range(64)] for c in range(3)]
        self.dc_tab, self.ac_tab = [d.dc_tab[c] for c in range(3)], [d.ac_tab[c] for c in range(3)]
        self.bits = [[d.bits[t][l] for l in range(16)] for t in range(4)]
        self.vals = [[d.vals[t][k] for k in range(256)] for t in range(4)]
        self.bpm = 1 if self.ncomp == 1 else (6 if self.ss == 2 else 3)
        mcu = 8 * self.ss
        self.mw, self.mh = -(-self.W // mcu), -(-self.H // mcu)
        self.nmcu = self.mw * self.mh
        self.R = self.dri if 0 < self.dri < self.nmcu else self.nmcu
        self.NI = -(-self.nmcu // self.R)
        self.comp_of_slot = [0] if self.ncomp == 1 else ([0, 0, 0, 0, 1, 2] if self.ss == 2 else [0, 1, 2])


# ----------------------------------------------------------------------------------------------------------- clean stream
def byte_class(s, q):
    """jd_class: 0 stays, 1 dropped, 2 dropped (second byte of RSTm), 3 dropped and not allowed"""
    c, run = s[q], 0
    while run < 8 and q > run and s[q - 1 - run] == 0xFF:
        run += 1
    if run & 1:
        return 1 if c == 0 else (2 if 0xD0 <= c <= 0xD7 else 3)
    if c == 0xFF:
        if q + 1 >= len(s):
            return 3
        return 0 if s[q + 1] == 0 else 1
    return 0


def clean_stream(scan, NI):
    """-> (clean bytes, interval starts [NI + 1] (None where no marker gave one), status)"""
    s = Checked(scan)
    ff = np.flatnonzero(np.frombuffer(scan, np.uint8) == 0xFF).tolist()
    special = {}
    for q in ff:                                   # only bytes at or behind an FF can be anything but 0
        for r in (q, q + 1):
            if r < len(s) and r not in special:
                special[r] = byte_class(s, r)
    clean, starts, status, ord_ = bytearray(), Checked([None] * (NI + 1)), 0, 0
    starts[0] = 0
    at = 0
    for q in sorted(special):
        c = special[q]
        if c == 0:
            continue
        clean += scan[at:q]
        at = q + 1
        if c == 2:
            if s[q] - 0xD0 != ord_ & 7:
                status |= S_RST_ORDER
            if ord_ + 1 < NI:
                starts[ord_ + 1] = len(clean)
            ord_ += 1
        elif c == 3:
            status |= S_MARKER
    clean += scan[at:]
    starts[NI] = len(clean)
    if ord_ != NI - 1:
        status |= S_RST_COUNT
    return bytes(clean), starts, status


# ---------------------------------------------------------------------------------------------------------------- entropy
class Tables:
    """the decode tables of one file as the kernel builds them: 9-bit first level, maxcode / valoff walk behind it"""

    def __init__(self, d):
        self.lut = [Checked([0] * 512) for _ in range(4)]
        self.maxcode = [Checked([-1] * 17) for _ in range(4)]
        self.valoff = [Checked([0] * 17) for _ in range(4)]
        self.vals = [Checked(v) for v in d.vals]
        for t in range(4):
            code, k = 0, 0
            for l in range(1, 17):
                n = d.bits[t][l - 1]
                self.valoff[t][l] = k - code
                for _ in range(n):
                    if l <= 9:
                        ent = (l << 8) | d.vals[t][k & 255]
                        first = code << (9 - l)
                        for f in range(1 << (9 - l)):
                            self.lut[t][(first + f) & 511] = ent
                    code += 1
                    k += 1
                self.maxcode[t][l] = code - 1 if n else -1
                code <<= 1
        self.slot_dc = Checked([d.dc_tab[c] & 1 for c in d.comp_of_slot])
        self.slot_ac = Checked([2 + (d.ac_tab[c] & 1) for c in d.comp_of_slot])


class Interval:
    """one restart interval's clean bytes with the kernel's bit reader: 32 bits at p, zero at and behind the end"""

    def __init__(self, data):
        self.nbits = 8 * len(data)
        b = np.frombuffer(data + b"\0" * 5, np.uint8).astype(np.int64)
        self.w40 = Checked(((b[:-4] << 32) | (b[1:-3] << 24) | (b[2:-2] << 16) | (b[3:-1] << 8) | b[4:]).tolist()) if len(data) else Checked([])

    def peek(self, p):
        if p >= self.nbits:
            return 0
        return (self.w40[p >> 3] >> (8 - (p & 7))) & 0xFFFFFFFF


def run(T, iv, end, bpm, p, b, k, coef=None, blk=0, nb=0):
    """jd_run: decode from (p, b, k) until p reaches `end` -> (p, b, k, blocks completed, bad).  coef: the write pass"""
    n, bad = 0, 0
    write = coef is not None
    while p < end:
        if write and blk >= nb:
            break
        v = iv.peek(p)
        t = T.slot_dc[b] if k == 0 else T.slot_ac[b]
        e = T.lut[t][v >> 23]
        ln, sym = e >> 8, e & 255
        if not e:
            for l in range(10, 17):
                code = v >> (32 - l)
                if code <= T.maxcode[t][l]:
                    sym, ln = T.vals[t][(T.valoff[t][l] + code) & 255], l
                    break
        if not ln:
            bad |= write
            p += 1
            continue
        p += ln
        s = sym & 15
        val = 0
        if s:
            m = ((v << ln) & 0xFFFFFFFF) >> (32 - s)
            val = m if m >> (s - 1) else m - (1 << s) + 1
        if k == 0:
            p += s
            if write:
                coef[blk * 64] = val
            k = 1
        elif s == 0:
            if sym >> 4 == 15:
                bad |= write and k + 16 > 63
                k += 16
            else:
                bad |= write and (sym >> 4) != 0
                k = 64
        else:
            k += sym >> 4
            p += s
            if k <= 63:
                if write:
                    coef[blk * 64 + k] = val
            else:
                bad |= write
            k += 1
        if k >= 64:
            k, b, n, blk = 0, (0 if b + 1 == bpm else b + 1), n + 1, blk + 1
    return p, b, k, n, int(bool(bad))


def decode_interval(T, data, nb, bpm, subseq_words):
    """The subsequence iteration, the block prefix and the write pass on one interval -> (coefficients [nb * 64] with DC
    DIFFERENCES, status bits, rounds, number of subsequences)."""
    iv = Interval(data)
    SB = 32 * (subseq_words or SUBSEQ_DEFAULT)
    nsub = max(1, -(-iv.nbits // SB))
    ends = [min(iv.nbits, (q + 1) * SB) for q in range(nsub)]
    E = Checked([(q * SB, 0, 0) for q in range(nsub)])
    X = Checked([None] * nsub)
    N = Checked([0] * nsub)
    dirty = Checked([True] * nsub)
    rounds = 0
    while True:
        for q in range(nsub):
            if dirty[q]:
                p, b, k, n, _ = run(T, iv, ends[q], bpm, *E[q])
                X[q], N[q], dirty[q] = (p, b, k), n, False
        rounds += 1
        changed = False
        for q in range(1, nsub):
            if X[q - 1] != E[q]:
                E[q], dirty[q], changed = X[q - 1], True, True
        if not changed:
            break
        assert rounds <= nsub + 1, "the iteration did not reach its fixed point"
    coef = Checked([0] * (nb * 64))
    blk, bad = 0, 0
    for q in range(nsub):
        bad |= run(T, iv, ends[q], bpm, *E[q], coef=coef, blk=blk, nb=nb)[4]
        blk += N[q]
    status = (S_CODE if bad else 0) | (S_BLOCKS if blk != nb else 0)
    return coef, status, rounds, nsub


def model_coefficients(d, blob, subseq_words=0):
    """-> (int64 [blocks][64] zigzag with DC VALUES, status, [rounds per interval], [subsequences per interval])"""
    scan = blob[d.scan_off:d.scan_off + d.scan_len]
    clean, starts, status = clean_stream(scan, d.NI)
    coefs = np.zeros((d.nmcu * d.bpm, 64), np.int64)
    rounds, nsubs = [], []
    if status:
        return coefs, status, rounds, nsubs
    T = Tables(d)
    for it in range(d.NI):
        nm = min(d.R, d.nmcu - it * d.R)
        nb = nm * d.bpm
        c, st, r, ns = decode_interval(T, clean[starts[it]:starts[it + 1]], nb, d.bpm, subseq_words)
        status |= st
        rounds.append(r)
        nsubs.append(ns)
        c = np.array(c, np.int64).reshape(nb, 64)
        comps = np.tile(np.array(d.comp_of_slot), nm)
        for comp in set(d.comp_of_slot):                      # DC: differences -> values per component, from 0 in every interval
            c[comps == comp, 0] = np.cumsum(c[comps == comp, 0])
        c = ((c + 32768) & 0xFFFF) - 32768                   # the array is int16 on the device
        coefs[it * d.R * d.bpm:it * d.R * d.bpm + nb] = c
    return coefs, status, rounds, nsubs


# ------------------------------------------------------------------------------------------------------------------ pixels
def _pass(x, shift):
    """libjpeg's jidctint on the last axis (CONST_BITS 13), descaled by `shift`"""
    i0, i1, i2, i3, i4, i5, i6, i7 = [x[..., n] for n in range(8)]
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) * 8192, (i0 - i4) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    r = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], -1)
    return (r + (1 << (shift - 1))) >> shift


def idct(blocks):
    """[n][8][8] dequantised, natural order -> samples 0 .. 255: columns first (descale 11), then rows (18)"""
    w = _pass(blocks.transpose(0, 2, 1), 11).transpose(0, 2, 1)
    return np.clip(_pass(w, 18) + 128, 0, 255)


def planes(d, coefs):
    nat = np.zeros_like(coefs)
    nat[:, J.ZIGZAG] = coefs
    nat = nat.reshape(d.mh, d.mw, d.bpm, 64)

    def q(c):
        t = np.zeros(64, np.int64)
        t[J.ZIGZAG] = d.qt[c]
        return t
    tile = lambda px: px.reshape(d.mh, d.mw, 8, 8).transpose(0, 2, 1, 3).reshape(d.mh * 8, d.mw * 8)
    if d.bpm != 6:
        return [tile(idct((nat[:, :, c] * q(c)).reshape(-1, 8, 8))) for c in range(d.ncomp)]
    y = idct((nat[:, :, :4] * q(0)).reshape(-1, 8, 8)).reshape(d.mh, d.mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(d.mh * 16, d.mw * 16)
    return [y] + [tile(idct((nat[:, :, 3 + c] * q(c)).reshape(-1, 8, 8))) for c in (1, 2)]


def fancy(c, H, W):
    """libjpeg's h2v2 fancy upsampling of a chroma plane to H x W; at most 2 samples wide: 2 x 2 replication"""
    ch, cw = -(-H // 2), -(-W // 2)
    c = c[:ch, :cw]
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, 0), 2, 1)[:H, :W]
    up, dn = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    rows = np.empty((2 * ch, cw), np.int64)
    rows[0::2], rows[1::2] = 3 * c + up, 3 * c + dn
    l, r = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    o = np.empty((2 * ch, 2 * cw), np.int64)
    o[:, 0::2], o[:, 1::2] = (3 * rows + l + 8) >> 4, (3 * rows + r + 7) >> 4
    return o[:H, :W]


def pixels(d, coefs, expand_grey=False, mirror=False):
    pl = planes(d, coefs)
    H, W = d.H, d.W
    if d.ncomp == 1:
        out = pl[0][:H, :W, None].astype(np.uint8)
        out = np.repeat(out, 3, axis=2) if expand_grey else out
    else:
        y = pl[0][:H, :W]
        cb, cr = (fancy(pl[1], H, W), fancy(pl[2], H, W)) if d.ss == 2 else (pl[1][:H, :W], pl[2][:H, :W])
        cb, cr = cb - 128, cr - 128
        r = y + ((91881 * cr + 32768) >> 16)
        b = y + ((116130 * cb + 32768) >> 16)
        g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
        out = np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
    return out[:, ::-1].copy() if mirror else out


def model_decode(d, blob, subseq_words=0, expand_grey=False, mirror=False):
    """the whole decoder -> (uint8 HWC, status, rounds per interval, subsequences per interval)"""
    coefs, status, rounds, nsubs = model_coefficients(d, blob, subseq_words)
    return pixels(d, coefs, expand_grey, mirror), status, rounds, nsubs
