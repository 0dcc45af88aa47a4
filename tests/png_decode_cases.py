"""PNG decode cases (a helper, not a test): hand-made PNG files with every knob of the format the decoder has to follow, the image
set, a Python parser, and a host model of the whole device decoder (csrc/png_decode.hip) in which every array index is checked.
The judge of pixels is always Pillow on the same bytes; the judge of the inflate is ``zlib.decompress``."""
import functools
import io
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as J  # noqa: E402

SIGNATURE = b"\x89PNG\r\n\x1a\n"
# PPST_PNG_E_* / PPST_PNG_S_* of include/ppst_hip.h
E_SIGNATURE, E_TRUNCATED, E_IHDR, E_DEPTH, E_COLOUR, E_INTERLACE, E_SIZE, E_TOO_LARGE, E_IDAT, E_IEND, E_APNG, E_METHOD = range(-201, -213, -1)
S_CRC, S_ZLIB, S_BTYPE, S_STORED, S_LENGTHS, S_CODE, S_DISTANCE, S_STREAM, S_ADLER, S_FILTER = (1 << k for k in range(10))
LANES = 1024                       # PD_INF_T: subsequences per window
DEFAULT_WORDS = 4                  # PD_SUBSEQ_DEFAULT
DEAD = 0xFFFFFFFF

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


# ------------------------------------------------------------------------------------------------------------- making files
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_rows(arr, filters):
    """arr (H,W,C) uint8 -> the filtered stream (bytes): row y gets filter ``filters[y % len(filters)]``"""
    H, W, C = arr.shape
    flat = arr.reshape(H, W * C).astype(np.int64)
    out = bytearray()
    prev = np.zeros(W * C, np.int64)
    for y in range(H):
        ft = filters[y % len(filters)]
        cur = flat[y]
        left = np.concatenate([np.zeros(C, np.int64), cur[:-C]]) if W * C > C else np.zeros(W * C, np.int64)
        ul = np.concatenate([np.zeros(C, np.int64), prev[:-C]]) if W * C > C else np.zeros(W * C, np.int64)
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - left
        elif ft == 2:
            f = cur - prev
        elif ft == 3:
            f = cur - ((left + prev) >> 1)
        else:
            pa, pb, pc = np.abs(prev - ul), np.abs(left - ul), np.abs(left + prev - 2 * ul)
            f = cur - np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        out.append(ft)
        out += (f & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE, "huffman": zlib.Z_HUFFMAN_ONLY}
MIXED = (4, 0, 1, 2, 3, 4, 4, 3, 1)


def cut(stream, idat_cuts):
    """the zlib stream as a list of IDAT payloads.  idat_cuts: "one"; "bytes" (every byte its own chunk); "zero" (a zero-length
    chunk in the middle); "header" (a cut after the first byte: the zlib header is split); or an int: pieces of that many bytes"""
    if idat_cuts == "one":
        return [stream]
    if idat_cuts == "bytes":
        return [stream[k:k + 1] for k in range(len(stream))]
    if idat_cuts == "zero":
        m = len(stream) // 2
        return [stream[:m], b"", stream[m:]]
    if idat_cuts == "header":
        return [stream[:1], stream[1:]]
    return [stream[k:k + idat_cuts] for k in range(0, len(stream), idat_cuts)] or [b""]


def wrap(H, W, C, pieces, extra=()):
    """signature + IHDR + ``extra`` chunks + one IDAT per piece + IEND"""
    colour = {1: 0, 3: 2, 4: 6}[C]
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, colour, 0, 0, 0))
    for kind, data in extra:
        out += chunk(kind, data)
    for p in pieces:
        out += chunk(b"IDAT", p)
    return out + chunk(b"IEND", b"")


def make_png(arr, filters=MIXED, level=6, strategy="default", idat_cuts="one", extra=()):
    """arr (H,W,C) uint8, C in (1, 3, 4) -> a PNG file built with zlib and struct: the filter byte of every row, the zlib level
    (0: stored blocks) and strategy, and where the zlib stream is cut into IDAT chunks are the caller's."""
    H, W, C = arr.shape
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, STRATEGIES[strategy])
    data = filter_rows(arr, filters)
    stream = co.compress(data) + co.flush()
    return wrap(H, W, C, cut(stream, idat_cuts), extra)


def pillow_png(arr, optimize=False):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(buf, format="PNG", optimize=optimize)
    return buf.getvalue()


def pillow_pixels(blob, mode=None):
    """Pillow's reading of the file as (H,W,C) uint8; raises what Pillow raises"""
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    im.load()
    if mode:
        im = im.convert(mode)
    a = np.asarray(im)
    return a.reshape(a.shape[0], a.shape[1], -1)


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nbits):                       # LSB first
        self.acc |= v << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, nbits):                      # a Huffman code: MSB first
        self.put(int(format(c, "0%db" % nbits)[::-1], 2), nbits)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def deflate_fixed(data, tokens):
    """a zlib stream of ONE fixed-Huffman block from a token list: ints are literals, (length, distance) pairs are matches
    (zlib itself never emits a distance above 32768 - 262).  ``data``: what the tokens stand for (its Adler-32 is the trailer)."""
    w = BitWriter()
    w.put(1, 1)
    w.put(1, 2)

    def lit(s):
        if s < 144:
            w.code(0x30 + s, 8)
        elif s < 256:
            w.code(0x190 + s - 144, 9)
        elif s < 280:
            w.code(s - 256, 7)
        else:
            w.code(0xC0 + s - 280, 8)
    for t in tokens:
        if isinstance(t, tuple):
            ln, d = t
            ls = max(k for k in range(29) if LBASE[k] <= ln) if ln < 258 else 28
            lit(257 + ls)
            w.put(ln - LBASE[ls], LEXT[ls])
            ds = max(k for k in range(30) if DBASE[k] <= d)
            w.code(ds, 5)
            w.put(d - DBASE[ds], DEXT[ds])
        else:
            lit(t)
    lit(256)
    return b"\x78\x9c" + w.done() + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)


@functools.lru_cache(None)
def far_match_png():
    """16 x 4095 grey, filter 0: a random block of 8 rows = 32768 stream bytes, then the same 8 rows again, coded as matches of
    length 258 at distance exactly 32768 (and one shorter one)."""
    rng = np.random.default_rng(11)
    block = rng.integers(0, 256, (8, 4095, 1), dtype=np.uint8)
    arr = np.concatenate([block, block], axis=0)
    data = filter_rows(arr, (0,))
    assert len(data) == 65536 and data[:32768] == data[32768:]
    tokens = list(data[:32768])
    left = 32768
    while left:
        ln = min(258, left)
        if 0 < left - ln < 3:
            ln -= 3
        tokens.append((ln, 32768))
        left -= ln
    stream = deflate_fixed(data, tokens)
    assert zlib.decompress(stream) == data
    return arr, wrap(16, 4095, 1, cut(stream, 8192))


# ---------------------------------------------------------------------------------------------------------------- image set
def label_map():
    rng = np.random.default_rng(13)
    return np.kron(rng.integers(0, 3, (8, 8), dtype=np.uint8), np.ones((16, 16), np.uint8))[:, :, None].copy()


@functools.lru_cache(None)
def image_set():
    """name -> (H,W,C) uint8, C in (1, 3, 4).  jpeg_cases.image_set() plus the shapes the PNG decoder can break at."""
    rng = np.random.default_rng(17)
    rnd = lambda H, W, C=3: rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    s = dict(J.image_set())
    s["1x70"], s["70x1"], s["1x1_rgba"] = rnd(1, 70), rnd(70, 1), rnd(1, 1, 4)
    s["63x5"], s["64x5_rgba"], s["65x5"] = J.field(21, 63, 5, 1.2, noise=1.0), rnd(64, 5, 4), J.field(22, 65, 5, 1.2, noise=1.0)   # the band edge
    s["130x67_grey"] = J.field(23, 130, 67, 1.3, noise=1.0)[:, :, :1].copy()       # three bands, two pieces of 64 pixels
    s["200x131_grey"] = J.field(24, 200, 131, 1.4, noise=1.0)[:, :, :1].copy()
    s["41x77_rgba"] = np.concatenate([J.field(3, 41, 77, 1.4, noise=1.0), rnd(41, 77, 1)], axis=2)
    s["600x530"] = J.field(25, 600, 530, 1.5, noise=1.5)
    s["field512"] = J.field(26, 512, 512, 1.4, noise=1.0)                          # the only large one
    s["const512"] = np.full((512, 512, 3), 77, np.uint8)                           # the longest distance-1 chains
    s["labels128"] = label_map()
    for v in s.values():
        v.setflags(write=False)
    return s


LARGE = ("600x530", "field512")                    # the host model walks these in a few settings only (it is Python)
SMALL_BYTES = 4096                                 # "every byte its own chunk" is made for files up to this many stream bytes

# family -> make_png's settings.  Every row filter forced, a mixed pattern; the levels (0: stored blocks); the strategies; the cuts.
FAMILIES = {
    "f0": dict(filters=(0,)), "f1": dict(filters=(1,)), "f2": dict(filters=(2,)), "f3": dict(filters=(3,)), "f4": dict(filters=(4,)),
    "mixed": dict(), "stored": dict(level=0), "level1": dict(level=1), "level9": dict(level=9),
    "fixed": dict(strategy="fixed"), "rle": dict(strategy="rle"), "huffman": dict(strategy="huffman"),
    "cut_bytes": dict(idat_cuts="bytes"), "cut_zero": dict(idat_cuts="zero"), "cut_header": dict(idat_cuts="header"),
    "cut_8192_trns": dict(idat_cuts=8192),
}
PILLOW_FAMILIES = ("pillow", "pillow_optimize")


@functools.lru_cache(None)
def family_files(family):
    """(names, blobs) of the whole image set in one family (+ the far-match file in "mixed")"""
    names, blobs = [], []
    for name, arr in sorted(image_set().items()):
        if family in PILLOW_FAMILIES:
            blob = pillow_png(arr, family == "pillow_optimize")
        else:
            kw = dict(FAMILIES[family])
            if kw.get("idat_cuts") == "bytes" and arr.size + arr.shape[0] > SMALL_BYTES:
                kw["idat_cuts"] = 4099                                   # (a prime: cuts fall anywhere in a token)
            if family == "cut_8192_trns" and arr.shape[2] != 4:          # an ancillary chunk Pillow ignores for the pixels, and a tEXt
                kw["extra"] = ((b"tRNS", b"\x00\x07" if arr.shape[2] == 1 else b"\x00\x01\x00\x02\x00\x03"), (b"tEXt", b"k\x00v"))
            blob = make_png(arr, **kw)
        names.append(name)
        blobs.append(blob)
    if family == "mixed":
        names.append("far_match")
        blobs.append(far_match_png()[1])
    return tuple(names), tuple(blobs)


def all_families():
    return list(FAMILIES) + list(PILLOW_FAMILIES)


# -------------------------------------------------------------------------------------------------------------- Python parser
def parse(blob, span_cap=None):
    """ppst_png_parse restated: (code, fields dict, spans list of (type, off, len, crc, idat))"""
    n = len(blob)
    d = dict(H=0, W=0, colour=0, channels=0, nspans=0, first_idat=0, nidat=0, idat_bytes=0, file_len=0)
    if n >= 0x10000000:
        return E_TOO_LARGE, d, []
    d["file_len"] = n
    for k in range(8):
        if k >= n:
            return E_TRUNCATED, d, []
        if blob[k] != SIGNATURE[k]:
            return E_SIGNATURE, d, []
    at, spans, first_idat, nidat, idat_bytes, iend, closed = 8, [], -1, 0, 0, False, False
    while not iend:
        if at == n:
            break
        if at + 8 > n:
            return E_TRUNCATED, d, spans
        ln, kind = struct.unpack(">I4s", blob[at:at + 8])
        if ln > 0x7FFFFFFF or at + 8 + ln + 4 > n:
            return E_TRUNCATED, d, spans
        data = at + 8
        if not spans:
            if kind != b"IHDR" or ln != 13:
                return E_IHDR, d, spans
            W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", blob[data:data + 13])
            if W == 0 or H == 0 or W > 0x7FFFFFFF or H > 0x7FFFFFFF:
                return E_SIZE, d, spans
            if colour not in (0, 2, 6):
                return E_COLOUR, d, spans
            if depth != 8:
                return E_DEPTH, d, spans
            if comp or filt:
                return E_METHOD, d, spans
            if lace:
                return E_INTERLACE, d, spans
            C = {0: 1, 2: 3, 6: 4}[colour]
            if 1 + W * C >= 1 << 31 or H * (1 + W * C) >= 1 << 31:
                return E_TOO_LARGE, d, spans
            d.update(H=H, W=W, colour=colour, channels=C)
        elif kind == b"IHDR":
            return E_IHDR, d, spans
        elif kind == b"acTL":
            return E_APNG, d, spans
        idat = kind == b"IDAT"
        if idat:
            if closed:
                return E_IDAT, d, spans
            if first_idat < 0:
                first_idat = len(spans)
            nidat += 1
            idat_bytes += ln
        elif first_idat >= 0:
            closed = True
        if kind == b"IEND":
            iend = True
        spans.append((struct.unpack(">I", kind)[0], data, ln, struct.unpack(">I", blob[data + ln:data + ln + 4])[0], int(idat)))
        at = data + ln + 4
    if not spans:
        return E_TRUNCATED, d, spans
    if not iend:
        return (E_IDAT if first_idat < 0 else E_IEND), d, spans
    if first_idat < 0:
        return E_IDAT, d, spans
    d.update(nspans=len(spans), first_idat=first_idat, nidat=nidat, idat_bytes=idat_bytes)
    return 0, d, spans


def refusal_files():
    """code -> a file the parser refuses with it"""
    arr = image_set()["17x3"]
    good = make_png(arr)
    ihdr = lambda **kw: struct.pack(">IIBBBBB", kw.get("W", 3), kw.get("H", 17), kw.get("depth", 8), kw.get("colour", 2), kw.get("comp", 0),
                                    kw.get("filt", 0), kw.get("lace", 0))
    body = good[33:]
    with_ihdr = lambda **kw: SIGNATURE + chunk(b"IHDR", ihdr(**kw)) + body
    idat_at = good.index(b"IDAT") - 4
    idat = good[idat_at:len(good) - 12]
    text = chunk(b"tEXt", b"a\x00b")
    return {
        E_SIGNATURE: b"\x89PNG\r\n\x1a\x0b" + good[8:],
        E_TRUNCATED: good[:len(good) - 5],
        E_IHDR: SIGNATURE + text + good[8:],
        E_DEPTH: with_ihdr(depth=16),
        E_COLOUR: with_ihdr(colour=3),
        E_INTERLACE: with_ihdr(lace=1),
        E_SIZE: with_ihdr(W=0),
        E_TOO_LARGE: with_ihdr(W=1 << 20, H=1 << 20),
        E_IDAT: good[:idat_at] + idat + text + idat + good[-12:],
        E_IEND: good[:-12],
        E_APNG: good[:33] + chunk(b"acTL", struct.pack(">II", 1, 0)) + body,
        E_METHOD: with_ihdr(comp=1),
    }


def more_refusals():
    """further files, with the code expected: the second reading of codes that have two"""
    arr = image_set()["17x3"]
    good = make_png(arr)
    return [(E_COLOUR, SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 3, 17, 8, 4, 0, 0, 0)) + good[33:]),
            (E_IHDR, SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 3, 17, 8, 2, 0, 0, 0) + b"\x00") + good[33:]),
            (E_IDAT, good[:33] + good[-12:]),
            (E_TRUNCATED, good[:8]), (E_TRUNCATED, b""), (E_TRUNCATED, good[:20]), (E_METHOD, SIGNATURE + chunk(
                b"IHDR", struct.pack(">IIBBBBB", 3, 17, 8, 2, 0, 1, 0)) + good[33:])]


# ------------------------------------------------------------------------------------------------------------------ the model
class Bounds(AssertionError):
    pass


def _ck(ok, what):
    if not ok:
        raise Bounds(what)


class Code:
    """one canonical code as the device holds it: lut (9 bits), sorted / count / first / index for the longer codes"""

    def __init__(self, lens, empty_ok):
        self.count = [0] * 16
        for l in lens:
            _ck(0 <= l < 16, "length")
            self.count[l] += 1
        self.first, self.index = [0] * 16, [0] * 16
        code, left, maxl, idx = 0, 1, 0, 0
        self.bad = False
        for l in range(1, 16):
            code = (code + (self.count[l - 1] if l > 1 else 0)) << 1
            self.first[l], self.index[l] = code, idx
            idx += self.count[l]
            left = (left << 1) - self.count[l]
            if left < 0:
                self.bad = True
                return
            if self.count[l]:
                maxl = l
        if maxl == 0:
            self.bad = not empty_ok
        elif left > 0 and maxl != 1:
            self.bad = True
        self.lut, self.sorted = [0] * 512, [0] * 288
        seen = [0] * 16
        for s, l in enumerate(lens):
            if not l:
                continue
            rank = seen[l]                                   # symbols of this length in front of s
            seen[l] += 1
            at = self.index[l] + rank
            _ck(0 <= at < 288, "sorted index")
            self.sorted[at] = s
            if l <= 9:
                rev = int(format(self.first[l] + rank, "0%db" % l)[::-1], 2)
                for f in range(1 << (9 - l)):
                    at = rev | (f << l)
                    _ck(0 <= at < 512, "lut index")
                    self.lut[at] = (l << 9) | s

    def sym(self, v):
        """(symbol, length) at the low end of the 32 bits v; (-1, 0): no such code"""
        e = self.lut[v & 511]
        if e:
            return e & 511, e >> 9
        rev = int(format(v & 0xFFFFFFFF, "032b")[::-1], 2)
        for l in range(10, 16):
            code = rev >> (32 - l)
            k = code - self.first[l]
            if 0 <= k < self.count[l]:
                at = self.index[l] + k
                _ck(0 <= at < 288, "sorted index")
                return self.sorted[at], l
        return -1, 0


class Inflate:
    """the device's inflate of one zlib stream ``zs`` into n bytes: blocks in order, per block the subsequence iteration in
    windows of LANES subsequences of 32 * words bits, prefix, write pass into raw / src.  Counts what the bounds speak of."""

    def __init__(self, zs, n, words=0):
        self.L, self.n = len(zs), n
        self.z = bytes(zs) + bytes(16)
        self.nbits = 8 * self.L
        self.SB = 32 * (words or DEFAULT_WORDS)
        self.raw = np.zeros(n, np.uint8)
        self.src = np.full(n, -1, np.int64)
        self.bits, self.outpos, self.final, self.p = 0, 0, False, 16
        self.blocks, self.max_rounds, self.windows, self.far, self.window_rounds = 0, 0, 0, 0, []
        self.tok = {}
        self.run()

    def peek(self, p):
        _ck(0 <= p < self.nbits + 64, "peek %d" % p)
        w = p >> 5
        _ck(4 * w + 8 <= len(self.z), "peek word")
        return (int.from_bytes(self.z[4 * w:4 * w + 8], "little") >> (p & 31)) & 0xFFFFFFFF

    def token(self, p):
        """(next p, kind, len, dist): kind 0 literal (value in len), 1 match, 2 end of block, 3 undefined"""
        t = self.tok.get(p)
        if t is not None:
            return t
        p0 = p
        v = self.peek(p)
        s, l = self.lit.sym(v)
        if s < 0:
            t = (p + 1, 3, 0, 0)
        else:
            p += l
            if s < 256:
                t = (p, 0, s, 0)
            elif s == 256:
                t = (p, 2, 0, 0)
            elif s > 285:
                t = (p, 3, 0, 0)
            else:
                eb = LEXT[s - 257]
                ln = LBASE[s - 257] + ((v >> l) & ((1 << eb) - 1))
                p += eb
                v = self.peek(p)
                ds, l = self.dist.sym(v)
                if ds < 0:
                    t = (p + 1, 3, 0, 0)
                elif ds > 29:
                    t = (p + l, 3, 0, 0)
                else:
                    p += l
                    db = DEXT[ds]
                    t = (p + db, 1, ln, DBASE[ds] + ((v >> l) & ((1 << db) - 1)))
        _ck(t[0] - p0 <= 48, "token longer than 48 bits")
        self.tok[p0] = t
        return t

    def stop(self, bit):
        self.bits |= bit
        return False

    def header(self):
        """the block header at self.p; False: stop"""
        p, nbits = self.p, self.nbits
        if p + 3 > nbits:
            return self.stop(S_STREAM)
        v = self.peek(p)
        self.bfinal, self.btype = v & 1, (v >> 1) & 3
        p += 3
        if self.btype == 3:
            return self.stop(S_BTYPE)
        if self.btype == 0:
            at = (p + 7) >> 3
            if at + 4 > self.L:
                return self.stop(S_STORED)
            ln, nl = self.z[at] | self.z[at + 1] << 8, self.z[at + 2] | self.z[at + 3] << 8
            if ln ^ 0xFFFF != nl or at + 4 + ln > self.L:
                return self.stop(S_STORED)
            self.st_at, self.st_len, self.p = at + 4, ln, (at + 4 + ln) * 8
            return True
        if self.btype == 1:
            self.lens, self.nl, self.nd, self.p = FIXED_LENS + [5] * 32, 288, 32, p
            return True
        if p + 14 > nbits:
            return self.stop(S_STREAM)
        v = self.peek(p)
        hlit, hdist, hclen = (v & 31) + 257, ((v >> 5) & 31) + 1, ((v >> 10) & 15) + 4
        p += 14
        if hlit > 286 or hdist > 30:
            return self.stop(S_LENGTHS)
        if p + 3 * hclen > nbits:
            return self.stop(S_STREAM)
        cl = [0] * 19
        for k in range(hclen):
            cl[CLORDER[k]] = self.peek(p) & 7
            p += 3
        left = 1
        for l in range(1, 8):
            left = (left << 1) - cl.count(l)
        if left != 0:
            return self.stop(S_LENGTHS)
        clc = Code(cl, False)
        total, lens, prev = hlit + hdist, [], 0
        while len(lens) < total:
            if p >= nbits:
                return self.stop(S_STREAM)
            v = self.peek(p)
            s, l = clc.sym(v)
            if s < 0 or l > 7:
                return self.stop(S_LENGTHS)
            p += l
            v >>= l
            if s < 16:
                rep, val = 1, s
            elif s == 16:
                if not lens:
                    return self.stop(S_LENGTHS)
                rep, val = 3 + (v & 3), prev
                p += 2
            elif s == 17:
                rep, val = 3 + (v & 7), 0
                p += 3
            else:
                rep, val = 11 + (v & 127), 0
                p += 7
            if len(lens) + rep > total:
                return self.stop(S_LENGTHS)
            lens += [val] * rep
            prev = val
        if p > nbits:
            return self.stop(S_STREAM)
        if lens[256] == 0:
            return self.stop(S_LENGTHS)
        self.lens = lens[:hlit] + [0] * (288 - hlit) + lens[hlit:] + [0] * (32 - hdist)
        self.nl, self.nd, self.p = hlit, hdist, p
        return True

    def decode(self, p, end, write_at=None):
        """from p until `end` or the end of the block: (exit or DEAD, bytes, eob position or None)"""
        cnt, pos = 0, write_at
        while p < end:
            p, kind, ln, d = self.token(p)
            if kind == 2:
                return DEAD, cnt, p
            if kind == 3:
                if write_at is not None:
                    self.bits |= S_CODE
                continue
            if kind == 0:
                if write_at is not None:
                    if pos < self.n:
                        _ck(0 <= pos, "raw store")
                        self.raw[pos], self.src[pos] = ln, pos
                    pos += 1
                cnt += 1
                continue
            if write_at is not None:
                far = d > pos
                if far:
                    self.bits |= S_DISTANCE
                if d == 32768 and ln == 258 and not far:
                    self.far += 1
                k = np.arange(ln)
                at = pos + k
                keep = at < self.n
                _ck(at[keep].size == 0 or (at[keep].min() >= 0 and at[keep].max() < self.n), "src store")
                if far:
                    self.raw[at[keep]], self.src[at[keep]] = 0, at[keep]
                else:
                    val = pos + (k % d) - d
                    _ck(val[keep].size == 0 or (val[keep].min() >= 0 and (val[keep] < at[keep]).all()), "src value")
                    self.src[at[keep]] = val[keep]
                pos += ln
            cnt += ln
        return p, cnt, None

    def run(self):
        nbits, SB = self.nbits, self.SB
        max_blocks = nbits // 3 + 1
        while self.blocks < max_blocks:
            self.blocks += 1
            if not self.header():
                return
            if self.btype == 0:
                if self.st_len > self.n - self.outpos:
                    return self.stop(S_STREAM)
                _ck(self.st_at + self.st_len <= self.L, "stored read")
                at = np.arange(self.outpos, self.outpos + self.st_len)
                self.raw[at] = np.frombuffer(self.z, np.uint8, self.st_len, self.st_at)
                self.src[at] = at
                self.outpos += self.st_len
            else:
                self.lit, self.dist = Code(self.lens[:self.nl], False), Code(self.lens[288:288 + self.nd], True)
                if self.lit.bad or self.dist.bad:
                    return self.stop(S_LENGTHS)
                self.tok = {}
                wstart = entry0 = self.p
                eob_p = None
                max_windows = (nbits - min(nbits, wstart)) // (SB * LANES) + 2
                for _ in range(max_windows):
                    if wstart >= nbits or entry0 >= nbits:
                        break
                    self.windows += 1
                    nact = min(LANES, (nbits - wstart + SB - 1) // SB)
                    ends = [min(nbits, wstart + (q + 1) * SB) for q in range(nact)]
                    entry = [entry0] + [wstart + q * SB for q in range(1, nact)]
                    res = [None] * nact
                    dirty = set(range(nact))
                    rounds = 0
                    while True:
                        for q in dirty:
                            res[q] = self.decode(entry[q], ends[q])
                        rounds += 1
                        dirty = set()
                        for q in range(1, nact):
                            if res[q - 1][0] != entry[q]:
                                entry[q] = res[q - 1][0]
                                if entry[q] == DEAD:
                                    # behind the block's end: nothing to decode, nothing to hand on (the exit stays what it
                                    # was), no part in the fixed point
                                    res[q] = (res[q][0], 0, None)
                                else:
                                    dirty.add(q)
                        if not dirty:
                            break
                        _ck(rounds <= nact, "more rounds than subsequences")
                    _ck(rounds <= nact, "more rounds than subsequences")
                    self.max_rounds = max(self.max_rounds, rounds)
                    self.window_rounds.append(rounds)
                    eobs = [q for q in range(nact) if res[q][2] is not None]
                    last = eobs[0] if eobs else nact - 1         # the chain is exact up to the first end-of-block
                    for q in range(1, last + 1):
                        _ck(entry[q] == res[q - 1][0] and entry[q] != DEAD, "the chain is not at its fixed point")
                    total = sum(r[1] for r in res[:last + 1])
                    if total > self.n - self.outpos:
                        return self.stop(S_STREAM)
                    pos = self.outpos
                    for q in range(last + 1):
                        again = self.decode(entry[q], ends[q], write_at=pos)
                        _ck(again == res[q], "the write pass walked another way")
                        pos += res[q][1]
                    self.outpos += total
                    if eobs:
                        eob_p = res[eobs[0]][2]
                        break
                    entry0 = res[nact - 1][0]
                    wstart += SB * LANES
                if eob_p is None:
                    return self.stop(S_STREAM)
                self.p = eob_p
            if self.bfinal:
                self.final = True
                break
        if not self.bits and (not self.final or self.outpos != self.n):
            self.bits |= S_STREAM


def sequential_inflate(zs):
    """a plain one-token-at-a-time inflate of a zlib stream with the model's own tables (no subsequences): bytes"""
    inf = Inflate.__new__(Inflate)
    inf.L, inf.z, inf.nbits, inf.bits, inf.p, inf.tok = len(zs), bytes(zs) + bytes(16), 8 * len(zs), 0, 16, {}
    out = bytearray()
    while True:
        assert inf.header(), inf.bits
        if inf.btype == 0:
            out += inf.z[inf.st_at:inf.st_at + inf.st_len]
        else:
            inf.lit, inf.dist, inf.tok = Code(inf.lens[:inf.nl], False), Code(inf.lens[288:288 + inf.nd], True), {}
            assert not inf.lit.bad and not inf.dist.bad
            p = inf.p
            while True:
                p, kind, ln, d = inf.token(p)
                assert kind != 3
                if kind == 2:
                    break
                if kind == 0:
                    out.append(ln)
                else:
                    assert d <= len(out)
                    for _ in range(ln):
                        out.append(out[-d])
            inf.p = p
        if inf.bfinal:
            return bytes(out)


def jump_rounds(src, seed=0):
    """pointer jumping src[i] <- src[src[i]] in place until a round changes nothing, in a deliberately adversarial order: every
    round a fresh random permutation, applied in 7 pieces one after the other, so reads see a mix of old and new values.
    -> rounds run, the last (which changes nothing) included"""
    n = src.size
    rng = np.random.default_rng(seed)
    rounds = 0
    while True:
        rounds += 1
        changed = False
        perm = rng.permutation(n)
        for piece in np.array_split(perm, 7):
            a = src[piece]
            _ck(a.size == 0 or (a.min() >= 0 and a.max() < n), "src index")
            b = src[a]
            _ck(b.size == 0 or (b.min() >= 0 and b.max() < n), "src index")
            if (a != b).any():
                changed = True
                src[piece] = b
        if not changed:
            return rounds
        _ck(rounds <= 40, "pointer jumping does not end")


def adler32(stream):
    """by the device's pieces of 4096 bytes: (A, B) partial sums joined in order"""
    a, b = 1, 0
    for c0 in range(0, len(stream), 4096):
        piece = np.frombuffer(stream, np.uint8, min(4096, len(stream) - c0), c0).astype(np.int64)
        m = piece.size
        pa, pb = int(piece.sum()) % 65521, int(((m - np.arange(m)) * piece).sum()) % 65521
        b = (b + m * a + pb) % 65521
        a = (a + pa) % 65521
    return (b << 16) | a


def unfilter(stream, H, W, C):
    """the device's skew, vectorised over the rows: at step t row y undoes pixel x = t - y, with the pixel above from row y - 1's
    step t - 1.  -> ((H,W,C) uint8, a filter byte above 4 seen)"""
    row = 1 + W * C
    buf = np.frombuffer(stream, np.uint8).reshape(H, row)
    ft = buf[:, 0].astype(np.int64)
    px = buf[:, 1:].reshape(H, W, C).astype(np.int64)
    rec = np.zeros((H + 1, W + 1, C), np.int64)            # row 0 and column 0: the zeros above and to the left
    ys = np.arange(H)
    for t in range(H + W - 1):
        xs = t - ys
        ok = (xs >= 0) & (xs < W)
        y, x = ys[ok], xs[ok]
        a, b, c = rec[y + 1, x], rec[y, x + 1], rec[y, x]
        f = ft[y][:, None]
        pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        add = np.where(f == 1, a, np.where(f == 2, b, np.where(f == 3, (a + b) >> 1, np.where(f == 4, paeth, 0))))
        rec[y + 1, x + 1] = (px[y, x] + add) & 255
    return rec[1:, 1:].astype(np.uint8), bool((ft > 4).any())


class Decoded:
    pass


def model_decode(blob, d, spans, words=0, expand_grey=False, drop_alpha=False, mirror=False):
    """the whole device decoder on one accepted file -> Decoded: status, pixels ((H,W,C') uint8 or None), and the counts the
    bounds speak of (rounds, jump_rounds, blocks, far)"""
    out = Decoded()
    out.status, out.pixels, out.rounds, out.jump_rounds, out.blocks, out.far, out.stream = 0, None, 0, 0, 0, 0, None
    n_file = len(blob)
    zs = bytearray()
    for kind, off, ln, crc, idat in spans:
        _ck(off >= 4 and ln >= 0 and off + ln + 4 <= n_file, "span outside the file")
        if zlib.crc32(blob[off - 4:off + ln]) & 0xFFFFFFFF != crc:
            out.status |= S_CRC
        if idat:
            zs += blob[off:off + ln]
    _ck(len(zs) == d["idat_bytes"], "idat_bytes")
    if len(zs) < 2 or (zs[0] & 15) != 8 or (zs[0] >> 4) > 7 or (zs[1] & 32) or ((zs[0] << 8) | zs[1]) % 31:
        out.status |= S_ZLIB
    if out.status:
        return out
    H, W, C = d["H"], d["W"], d["channels"]
    n = H * (1 + W * C)
    inf = Inflate(zs, n, words)
    out.rounds, out.blocks, out.far, out.inflate = inf.max_rounds, inf.blocks, inf.far, inf
    _ck(inf.blocks <= 8 * len(zs) // 3 + 1, "more blocks than bits / 3")
    out.status |= inf.bits
    if out.status:
        return out
    _ck((inf.src >= 0).all(), "a byte of the stream was not written")
    out.jump_rounds = jump_rounds(inf.src)
    stream = inf.raw[inf.src].tobytes()
    out.stream = stream
    at = (inf.p + 7) >> 3
    if at + 4 > len(zs) or adler32(stream) != struct.unpack(">I", bytes(zs[at:at + 4]))[0]:
        out.status |= S_ADLER
    px, bad = unfilter(stream, H, W, C)
    if bad:
        out.status |= S_FILTER
    if C == 1 and expand_grey:
        px = np.repeat(px, 3, axis=2)
    if C == 4 and drop_alpha:
        px = px[:, :, :3]
    out.pixels = px[:, ::-1].copy() if mirror else px
    return out


def log2_ceil(n):
    return max(0, (n - 1).bit_length())


# --------------------------------------------------------------------------------------------------------- robustness corpus
def corpus_base():
    """one small file with three IDAT chunks, dynamic blocks with matches, every filter"""
    arr = J.field(31, 24, 20, 1.3, noise=0.5)
    arr = np.concatenate([arr, arr[:8]], axis=0)
    return make_png(arr, idat_cuts=150, extra=((b"tEXt", b"key\x00value"),))


def _recrc(blob):
    """every chunk's CRC recomputed (where the chunk structure can still be walked)"""
    out, at = bytearray(blob), 8
    while at + 12 <= len(out):
        ln = struct.unpack(">I", out[at:at + 4])[0]
        if at + 12 + ln > len(out):
            break
        out[at + 8 + ln:at + 12 + ln] = struct.pack(">I", zlib.crc32(bytes(out[at + 4:at + 8 + ln])) & 0xFFFFFFFF)
        at += 12 + ln
    return bytes(out)


@functools.lru_cache(None)
def corpus():
    """[(name, bytes)]: every prefix of the base file; 200 single-byte corruptions of its chunk data; 200 more with the chunk
    CRCs recomputed"""
    base = corpus_base()
    files = [("prefix%d" % k, base[:k]) for k in range(len(base))]
    rc, d, spans = parse(base)
    assert rc == 0
    data_at = [off + k for _, off, ln, _, _ in spans for k in range(ln)]
    rng = np.random.default_rng(41)
    for fixed in (False, True):
        for k in range(200):
            at = data_at[int(rng.integers(0, len(data_at)))]
            v = int(rng.integers(1, 256))
            bad = base[:at] + bytes([base[at] ^ v]) + base[at + 1:]
            files.append(("flip%d%s" % (k, "_crc" if fixed else ""), _recrc(bad) if fixed else bad))
    return files


def damaged_files(good):
    """three damaged versions of one good single-IDAT-run file: a bad chunk CRC; a bad Adler-32 with the CRC fixed; the zlib
    stream cut short with the CRC fixed"""
    rc, d, spans = parse(good)
    assert rc == 0
    first = spans[d["first_idat"]]
    last = spans[d["first_idat"] + d["nidat"] - 1]
    at = first[1] + first[2] // 2
    bad_crc = good[:at] + bytes([good[at] ^ 0x5A]) + good[at + 1:]
    end = last[1] + last[2]
    assert last[2] >= 8
    bad_adler = _recrc(good[:end - 1] + bytes([good[end - 1] ^ 1]) + good[end:])
    head = good[:first[1] - 8]
    zs = b"".join(good[s[1]:s[1] + s[2]] for s in spans if s[4])
    truncated = head + chunk(b"IDAT", zs[:len(zs) // 2]) + chunk(b"IEND", b"")
    return bad_crc, bad_adler, truncated


def dump_corpus(directory):
    """the robustness corpus, the refusal files and one file of every family as files of a directory: what tests/png_parse_san.cpp
    walks"""
    os.makedirs(directory, exist_ok=True)
    files = list(corpus()) + [("refusal%d" % -c, b) for c, b in refusal_files().items()]
    files += [("more%d" % k, b) for k, (_, b) in enumerate(more_refusals())]
    files += [("set_%s" % fam, family_files(fam)[1][family_files(fam)[0].index("17x3")]) for fam in all_families()]
    for name, blob in files:
        with open(os.path.join(directory, name + ".png"), "wb") as f:
            f.write(blob)
    return len(files)
