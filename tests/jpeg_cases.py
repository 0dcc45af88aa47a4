"""The JPEG encoder's cases and judges (host-only numpy; no test in here): the image set, a float64 model of the format
include/ppst_hip.h states for ppst_jpeg_*, an entropy decoder (segments, Huffman-decode of the scan back to quantised
coefficients), an entropy encoder over given coefficients, and an integer emulation of the kernels' DCT for its error bound.
Everything restates the specification (ITU-T T.81 Annex K tables included); nothing calls the library under test.

Blocks are handled in SCAN order: MCUs in raster order, inside a 4:2:0 MCU Y00 Y01 Y10 Y11 Cb Cr, inside a 4:4:4 MCU Y Cb Cr.
Coefficients are int arrays [blocks][64] in zigzag order.
"""
import functools
import re
import struct

import numpy as np

# ------------------------------------------------------------------------------------------------------------ T.81 Annex K
QBASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32])
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
DC_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = [list(range(12)), list(range(12))]
AC_BITS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]]
_AC_TAIL = [r << 4 | s for r in range(2, 16) for s in range(1, 11)]          # not the tables: only a check of their 162 symbols
AC_VALS = [
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]]
assert all(len(v) == 162 == sum(b) and set(_AC_TAIL) <= set(v) for v, b in zip(AC_VALS, AC_BITS))

SUBSAMPLINGS = ("4:4:4", "4:2:0")
SS_NUMBER = {"4:4:4": 0, "4:2:0": 2}             # PPST_JPEG_444 / PPST_JPEG_420
QUALITIES = (5, 50, 90, 100)
BLOCKS_PER_INTERVAL = 96                         # the device encoder's DRI in blocks (JPEG_NBLK of csrc/jpeg.hip)
BLOCK_BITS = 11 + 11 + 63 * (16 + 10)            # longest DC code + 11 magnitude bits, 63 x (longest AC code + 10 bits)


def qtables(quality):
    """libjpeg's scaling: [2][64] natural order, luma and chroma."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((QBASE * s + 50) // 100, 1, 255)


def huff_codes(bits, vals):
    """T.81 Annex C: symbol -> (length, code)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (length, code)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [huff_codes(DC_BITS[t], DC_VALS[t]) for t in (0, 1)]
AC_CODES = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]
assert max(l for t in DC_CODES for l, _ in t.values()) == 11 and max(l for t in AC_CODES for l, _ in t.values()) == 16


def layout(C, subsampling):
    """-> (ss, blocks per MCU, component of each block of an MCU)."""
    if C == 1:
        return 1, 1, [0]
    return (2, 6, [0, 0, 0, 0, 1, 2]) if subsampling == "4:2:0" else (1, 3, [0, 1, 2])


def dri_mcus(C, subsampling):
    return BLOCKS_PER_INTERVAL // layout(C, subsampling)[1]


def header_len(C):
    n, t = (1, 1) if C == 1 else (3, 2)
    return 2 + 18 + 69 * t + (10 + 3 * n) + (33 + 183) * t + 6 + (8 + 2 * n)


def worst_case_bytes(H, W, C, subsampling, R=None):
    """The derivation of ppst_jpeg_bound: per block BLOCK_BITS bits; per restart interval the bits padded to a byte, every byte
    an FF followed by its 00 (x 2), and the marker behind it (RSTm, EOI behind the last); the header in front."""
    ss, bpm, _ = layout(C, subsampling)
    R = R or dri_mcus(C, subsampling)
    nmcu = -(-W // (8 * ss)) * -(-H // (8 * ss))
    total = header_len(C)
    for m0 in range(0, nmcu, R):
        nb = min(R, nmcu - m0) * bpm
        total += 2 * -(-nb * BLOCK_BITS // 8) + 2
    return total


# --------------------------------------------------------------------------------------------------------------- samples
def scan_blocks(arr, subsampling):
    """HWC uint8 -> (int64 [blocks][8][8] level-shifted samples in scan order, component of each block)."""
    H, W, C = arr.shape
    ss, bpm, comps = layout(C, subsampling)
    mcu = 8 * ss
    Hp, Wp = -(-H // mcu) * mcu, -(-W // mcu) * mcu
    p = np.pad(arr.astype(np.int64), ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge")        # edge replication
    mh, mw = Hp // mcu, Wp // mcu
    if C == 1:
        planes = [p[:, :, 0]]
    else:
        r, g, b = p[:, :, 0], p[:, :, 1], p[:, :, 2]
        planes = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                  (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                  (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]
        if ss == 2:
            bias = np.tile(np.array([1, 2]), Wp // 4)[None, :]
            for c in (1, 2):
                q = planes[c]
                planes[c] = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + bias) >> 2
    tiles = lambda q: q.reshape(q.shape[0] // 8, 8, q.shape[1] // 8, 8).transpose(0, 2, 1, 3)
    per = []
    if ss == 2:
        y = tiles(planes[0]).reshape(mh, 2, mw, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(mh * mw, 4, 8, 8)
        per = [y[:, 0], y[:, 1], y[:, 2], y[:, 3]] + [tiles(planes[c]).reshape(mh * mw, 8, 8) for c in (1, 2)]
    else:
        per = [tiles(q).reshape(mh * mw, 8, 8) for q in planes]
    blocks = np.stack(per, axis=1).reshape(mh * mw * bpm, 8, 8) - 128
    return blocks, np.tile(np.array(comps), mh * mw)


_u = np.arange(8)
DCT64 = np.where(_u[:, None] == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * _u[None, :] + 1) * _u[:, None] * np.pi / 16)      # [u][x]
DCT_INT = np.rint(DCT64 * (1 << 14)).astype(np.int64)


def dct_f64(blocks):
    """float64 8 x 8 DCT-II in JPEG's normalisation, [n][v][u]."""
    return DCT64 @ blocks.astype(np.float64) @ DCT64.T


def dct_fixed(blocks):
    """The kernels' arithmetic in int64: rows a = (sum s T + 128) >> 8, columns b = sum a T, scale 2^20 -> int64 [n][v][u]."""
    a = (np.einsum("nyx,ux->nyu", blocks, DCT_INT) + 128) >> 8
    assert np.abs(a).max() < 32768
    b = np.einsum("nyu,vy->nvu", a, DCT_INT)
    assert np.abs(b).max() < 2 ** 31 - (255 << 19)
    return b


# The absolute error of that arithmetic against float64, in coefficient units, over every image of image_set() and both
# subsamplings (test_jpeg_cases_cpu.test_fixed_point_dct_error_is_what_is_stated measures it again):
# (the largest errors are DC terms of flat and checkerboard blocks: the table's 5793 stands for 5792.62, twice, times 1024)
EPS_MEASURED = 0.1352          # the maximum found
EPS = 0.2704                   # the bound the coefficient test uses: twice that


def quantise(c, q_nat):
    """float or scale-2^20 integer coefficients [n][v][u], q_nat [n][64] -> int [n][64] zigzag; to nearest, halves away from 0."""
    q = q_nat.reshape(-1, 8, 8)
    if c.dtype.kind == "i":
        d = q.astype(np.int64) << 20
        v = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    else:
        v = np.sign(c) * np.floor(np.abs(c) / q + 0.5)
    return v.astype(np.int64).reshape(-1, 64)[:, ZIGZAG]


def block_q(comps, quality):
    """[blocks][64] natural order: the table of each block's component."""
    return qtables(quality)[np.minimum(comps, 1)]


# --------------------------------------------------------------------------------------------------------- entropy coding
def _size(v):
    return int(abs(v)).bit_length()


def entropy_encode(coefs, C, subsampling, R):
    """zigzag coefficients [blocks][64] in scan order -> the scan's bytes (behind SOS, in front of EOI): intervals of R MCUs, DC
    predictors from 0 in each, 1-bits to the byte boundary, FF -> FF 00, RSTm between intervals."""
    _, bpm, comps = layout(C, subsampling)
    out = bytearray()
    nblocks = len(coefs)
    rows = coefs.tolist()
    for i, j0 in enumerate(range(0, nblocks, R * bpm)):
        acc, n = 0, 0
        pred = [0, 0, 0]
        for j in range(j0, min(j0 + R * bpm, nblocks)):
            comp = comps[j % bpm]
            t = min(comp, 1)
            blk = rows[j]
            d = blk[0] - pred[comp]
            pred[comp] = blk[0]
            s = _size(d)
            l, c = DC_CODES[t][s]
            acc = (((acc << l) | c) << s) | ((d if d >= 0 else d - 1) & ((1 << s) - 1))
            n += l + s
            run = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    l, c = AC_CODES[t][0xF0]
                    acc = (acc << l) | c
                    n += l
                    run -= 16
                s = _size(v)
                l, c = AC_CODES[t][run << 4 | s]
                acc = (((acc << l) | c) << s) | ((v if v >= 0 else v - 1) & ((1 << s) - 1))
                n += l + s
                run = 0
            if run:
                l, c = AC_CODES[t][0x00]
                acc = (acc << l) | c
                n += l
        pad = -n % 8
        acc = (acc << pad) | ((1 << pad) - 1)
        if i:
            out += bytes([0xFF, 0xD0 + (i - 1) % 8])
        out += acc.to_bytes((n + pad) // 8, "big").replace(b"\xff", b"\xff\x00")
    return bytes(out)


def header(H, W, C, quality, subsampling, R):
    """SOI, APP0 (JFIF 1.01, density 1:1), DQT x 1 | 2, SOF0, DHT x 2 | 4, DRI, SOS."""
    ss, _, _ = layout(C, subsampling)
    nc, nt = (1, 1) if C == 1 else (3, 2)
    q = qtables(quality)
    o = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for t in range(nt):
        o += b"\xff\xdb" + struct.pack(">HB", 67, t) + bytes(q[t][ZIGZAG].tolist())
    o += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * nc, 8, H, W, nc)
    for c in range(nc):
        o += bytes([c + 1, (ss << 4 | ss) if c == 0 else 0x11, min(c, 1)])
    for t in range(nt):
        o += b"\xff\xc4" + struct.pack(">HB", 19 + 12, t) + bytes(DC_BITS[t]) + bytes(DC_VALS[t])
        o += b"\xff\xc4" + struct.pack(">HB", 19 + 162, 0x10 | t) + bytes(AC_BITS[t]) + bytes(AC_VALS[t])
    o += b"\xff\xdd" + struct.pack(">HH", 4, R)
    o += b"\xff\xda" + struct.pack(">HB", 6 + 2 * nc, nc)
    for c in range(nc):
        o += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return o + bytes([0, 63, 0])


def model_coefficients(arr, quality, subsampling):
    blocks, comps = scan_blocks(arr, subsampling)
    return quantise(dct_f64(blocks), block_q(comps, quality))


def model_encode(arr, quality, subsampling, R=None):
    """The float64 model's complete file (R: MCUs per restart interval; default the device encoder's)."""
    H, W, C = arr.shape
    R = R or dri_mcus(C, subsampling)
    return (header(H, W, C, quality, subsampling, R) + entropy_encode(model_coefficients(arr, quality, subsampling), C, subsampling, R)
            + b"\xff\xd9")


# --------------------------------------------------------------------------------------------------------------- decoding
def parse(blob):
    """-> dict: segments in order ("order": marker bytes), "dqt" {id: [64] zigzag}, "dht" {(class, id): payload bytes}, "sof"
    (precision, H, W, [(id, h, v, tq)]), "dri", "sos" [(id, td, ta)], "head" bytes through SOS, "scan" bytes up to EOI."""
    assert blob[:2] == b"\xff\xd8" and blob[-2:] == b"\xff\xd9"
    out = {"order": [0xD8], "dqt": {}, "dht": {}, "dri": 0}
    at = 2
    while True:
        assert blob[at] == 0xFF, "marker expected at byte %d" % at
        m = blob[at + 1]
        n, = struct.unpack(">H", blob[at + 2:at + 4])
        body = blob[at + 4:at + 2 + n]
        assert len(body) == n - 2
        out["order"].append(m)
        if m == 0xE0:
            out["app0"] = body
        elif m == 0xDB:
            i = 0
            while i < len(body):
                assert body[i] >> 4 == 0, "8-bit tables only"
                out["dqt"][body[i] & 15] = list(body[i + 1:i + 65])
                i += 65
        elif m == 0xC0:
            prec, H, W, nc = struct.unpack(">BHHB", body[:6])
            out["sof"] = (prec, H, W, [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nc)])
        elif m == 0xC4:
            i = 0
            while i < len(body):
                cnt = sum(body[i + 1:i + 17])
                out["dht"][(body[i] >> 4, body[i] & 15)] = bytes(body[i + 1:i + 17 + cnt])
                i += 17 + cnt
        elif m == 0xDD:
            out["dri"], = struct.unpack(">H", body)
        elif m == 0xDA:
            nc = body[0]
            out["sos"] = [(body[1 + 2 * c], body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(nc)]
            assert bytes(body[1 + 2 * nc:]) == bytes([0, 63, 0])
            at += 2 + n
            break
        else:
            raise AssertionError("unexpected marker FF%02X" % m)
        at += 2 + n
    out["head"], out["scan"] = blob[:at], blob[at:-2]
    return out


def _lut(table_payload):
    """DHT payload (16 counts + symbols) -> two lists over every 16-bit window: code length (0: no code), symbol."""
    codes = huff_codes(list(table_payload[:16]), list(table_payload[16:]))
    ln, sy = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    for sym, (l, c) in codes.items():
        ln[c << (16 - l):(c + 1) << (16 - l)] = l
        sy[c << (16 - l):(c + 1) << (16 - l)] = sym
    return ln.tolist(), sy.tolist()


def entropy_decode(blob):
    """A complete file -> (zigzag coefficients int64 [blocks][64] in scan order, the dict of parse()).  Checks on the way: every
    code is one of the file's DHT tables, intervals hold DRI MCUs, the RST markers count 0 .. 7 cyclically, FF is followed by 00
    inside an interval, the bits behind an interval's last block are fewer than 8 and all ones."""
    p = parse(blob)
    _, H, W, comps_sof = p["sof"]
    C = len(comps_sof)
    ss = comps_sof[0][1]
    assert comps_sof[0][1] == comps_sof[0][2] and all(c[1:3] == (1, 1) for c in comps_sof[1:])
    bpm = 1 if C == 1 else (6 if ss == 2 else 3)
    comps = [0] if C == 1 else ([0, 0, 0, 0, 1, 2] if ss == 2 else [0, 1, 2])
    nmcu = -(-W // (8 * ss)) * -(-H // (8 * ss))
    R = p["dri"] or nmcu
    luts = {key: _lut(v) for key, v in p["dht"].items()}
    tabs = [(luts[(0, td)], luts[(1, ta)]) for _, td, ta in p["sos"]]
    scan = p["scan"]
    marks = list(re.finditer(rb"\xff[^\x00]", scan))
    assert [m.group()[1] for m in marks] == [0xD0 + i % 8 for i in range(len(marks))], "RST markers out of order"
    cuts = [0] + [m.start() for m in marks] + [len(scan)]
    assert len(cuts) - 1 == -(-nmcu // R), "intervals: %d, expected %d" % (len(cuts) - 1, -(-nmcu // R))
    coefs = np.zeros((nmcu * bpm, 64), np.int64)
    j = 0
    for i in range(len(cuts) - 1):
        seg = scan[cuts[i] + (2 if i else 0):cuts[i + 1]]
        assert seg.count(b"\xff") == seg.count(b"\xff\x00")
        data = seg.replace(b"\xff\x00", b"\xff")
        nbits = 8 * len(data)
        b = np.frombuffer(data + b"\0\0\0\0", np.uint8).astype(np.int64)
        w32 = ((b[:-3] << 24) | (b[1:-2] << 16) | (b[2:-1] << 8) | b[3:]).tolist()
        at = 0
        pred = [0, 0, 0]
        for _ in range(min(R, nmcu - i * R) * bpm):
            comp = comps[j % bpm]
            (dl, ds), (al, as_) = tabs[comp]
            row = coefs[j]
            pk = (w32[at >> 3] >> (16 - (at & 7))) & 0xFFFF
            assert dl[pk], "no DC code at bit %d of interval %d" % (at, i)
            s = ds[pk]
            at += dl[pk]
            if s:
                v = ((w32[at >> 3] >> (16 - (at & 7))) & 0xFFFF) >> (16 - s)
                at += s
                pred[comp] += v if v >> (s - 1) else v - (1 << s) + 1
            row[0] = pred[comp]
            k = 1
            while k < 64:
                pk = (w32[at >> 3] >> (16 - (at & 7))) & 0xFFFF
                assert al[pk], "no AC code at bit %d of interval %d" % (at, i)
                sym = as_[pk]
                at += al[pk]
                r, s = sym >> 4, sym & 15
                if s == 0:
                    if r == 15:
                        k += 16
                        continue
                    assert r == 0
                    break
                k += r
                assert k < 64, "run past the block"
                v = ((w32[at >> 3] >> (16 - (at & 7))) & 0xFFFF) >> (16 - s)
                at += s
                row[k] = v if v >> (s - 1) else v - (1 << s) + 1
                k += 1
            j += 1
        assert 0 <= nbits - at < 8, "interval %d: %d bits behind its last block" % (i, nbits - at)
        if nbits > at:
            assert data[-1] & ((1 << (nbits - at)) - 1) == (1 << (nbits - at)) - 1, "pad bits are not ones"
    assert j == nmcu * bpm
    return coefs, p


# -------------------------------------------------------------------------------------------------------------- image set
def field(seed, H, W, alpha, corr=0.75, noise=0.0):
    """A seeded 1 / f^alpha colour field with correlated channels: a shared field and a smaller one per channel."""
    rng = np.random.default_rng([seed, 23])
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0

    def one():
        spec = np.fft.fft2(rng.standard_normal((H, W))) / f ** alpha
        spec[0, 0] = 0.0
        g = np.real(np.fft.ifft2(spec))
        return g / (g.std() + 1e-12)
    shared = one()
    out = np.empty((H, W, 3), np.uint8)
    for c in range(3):
        v = 128.0 + 44.0 * (corr * shared + (1 - corr) * one()) + noise * rng.standard_normal((H, W))
        out[:, :, c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out


def checker(period):
    y, x = np.mgrid[0:64, 0:64]
    return np.repeat((((y // period + x // period) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


@functools.lru_cache(None)
def image_set():
    """name -> HWC uint8: the smallest shapes at which each mechanism of the encoder can break."""
    rng = np.random.default_rng(7)
    rnd = lambda H, W, C=3: rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    s = {}
    s["1x1"], s["8x8"], s["16x16"] = rnd(1, 1), rnd(8, 8), rnd(16, 16)             # single MCU, exact MCU multiples
    s["1x1_grey"] = rnd(1, 1, 1)
    s["17x3"], s["41x77"] = rnd(17, 3), field(3, 41, 77, 1.4, noise=1.0)           # partial MCUs on both axes, odd chroma sizes
    s["160x136"] = field(4, 160, 136, 1.2, noise=2.0)                              # 11 intervals at 4:4:4: RSTm wraps
    s["200x232"] = field(5, 200, 232, 1.3, noise=1.0)                              # 13 intervals at 4:2:0 (28 at 4:4:4)
    s["8x2100"], s["2100x8"] = field(6, 8, 2100, 1.1, noise=2.0), field(7, 2100, 8, 1.1, noise=2.0)    # one MCU row / column
    s["64x700_grey"] = field(8, 64, 700, 1.3, noise=1.0)[:, :, :1].copy()          # grey path, wide: 8 intervals
    s["zeros"], s["ones"] = np.zeros((300, 200, 3), np.uint8), np.full((300, 200, 3), 255, np.uint8)   # DC only, EOB everywhere
    s["checker1"], s["checker8"] = checker(1), checker(8)                          # largest magnitudes: size categories 10 / 11
    s["random96"] = rnd(96, 96)                                                    # longest codes, dense FF stuffing at q 100
    s["random96_grey"] = rnd(96, 96, 1)
    s["smooth"] = field(9, 96, 136, 2.6)                                           # at q 5: long zero runs, ZRL chains
    s["photo96x136"], s["photo41x77"] = field(1, 96, 136, 1.4), field(2, 41, 77, 1.4)
    for v in s.values():
        v.setflags(write=False)
    return s


PHOTO = ("photo96x136", "photo41x77")            # + weights.synthetic_images at 256^2 where torch is at hand (synthetic256)


def synthetic256():
    import torch
    from ppst_amd import weights as W
    x = W.synthetic_images(21, 1, size=256)
    return ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()[0]


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / max(np.mean(d * d), 1e-12))


def pillow_encode(arr, quality, subsampling):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(buf, format="JPEG", quality=quality, subsampling=subsampling, optimize=False)
    return buf.getvalue()


def pillow_decode(blob):
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    im.load()
    a = np.asarray(im)
    return im.mode, im.size, a.reshape(a.shape[0], a.shape[1], -1)
