"""CPU restatement of the baseline JPEG that Pillow (libjpeg-turbo) writes for
an 8-bit RGB image with its defaults — the rule include/ipp.h states for
ipp_jpeg_encode — in NumPy for the per-sample arithmetic and plain Python for
the entropy coder.  `encode` returns the whole file and the coverage counters
the tests assert on (ZRL codes, blocks without EOB, stuffed 0xFF bytes, dummy
blocks, largest DC and AC category), so that a green comparison cannot hide a
path the inputs never took.  No Pillow call here: the tests compare these
bytes with `Image.save`'s."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

# Annex K.1 / K.2, natural (row-major) order
LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99], np.int64)

# natural index of zigzag position k
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)

# Annex K.3: (BITS[1..16], HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
    0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
    0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0,
    0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA])

SAMPLINGS = ("4:2:0", "4:4:4")


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """jpeg_set_quality(q, force_baseline): (luma, chroma), natural order."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (LUMA_Q, CHROMA_Q))


def huff_codes(spec) -> dict:
    """symbol -> (code, length) of a (BITS, HUFFVAL) table (Annex C)."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def header(w: int, h: int, quality: int, subsampling: str) -> bytes:
    """SOI, APP0 (JFIF 1.01, density 1:1 without unit), a DQT per table, SOF0,
    a DHT per table (DC0, AC0, DC1, AC1), SOS."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, t in enumerate(quant_tables(quality)):
        out += seg(0xDB, bytes([i]) + bytes(int(t[z]) for z in ZIGZAG))
    hv = 0x22 if subsampling == "4:2:0" else 0x11
    out += seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") +
               bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([tc_th]) + bytes(spec[0]) + bytes(spec[1]))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def rgb_to_ycc(a: np.ndarray) -> np.ndarray:
    """jccolor.c rgb_ycc_convert: 16-bit fixed point, (h, w, 3) int64."""
    r, g, b = (a[..., c].astype(np.int64) for c in range(3))
    half, off = 32768, 128 * 65536 + 32767
    y = (19595 * r + 38470 * g + 7471 * b + half) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + off) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + off) >> 16
    return np.stack([y, cb, cr], axis=-1)


def _pad_edge(p: np.ndarray, hh: int, ww: int) -> np.ndarray:
    """expand_right_edge / expand_bottom_edge: repeat the last column and row."""
    return np.pad(p, ((0, hh - p.shape[0]), (0, ww - p.shape[1])), mode="edge")


def component_planes(a: np.ndarray, subsampling: str) -> List[np.ndarray]:
    """The three components on their own block grids (⌈size / 8⌉ blocks: dummy
    blocks are not here).  4:2:0, as libjpeg orders it: the colour planes'
    columns are edge-replicated to the chroma grid's 16-px cells and their rows
    to an even count only (one row group), then h2v2_downsample with its
    alternating bias 1, 2 along a row, and then the last *chroma* row is
    repeated down to the block grid — for an even height that is not the
    downsample of a repeated pixel row."""
    h, w = a.shape[:2]
    ycc = rgb_to_ycc(a)
    up8 = lambda v: (v + 7) // 8 * 8
    if subsampling == "4:4:4":
        return [_pad_edge(ycc[..., c], up8(h), up8(w)) for c in range(3)]
    out = [_pad_edge(ycc[..., 0], up8(h), up8(w))]
    rows, cw = (h + 1) // 2, up8((w + 1) // 2)
    bias = np.where(np.arange(cw) % 2 == 0, 1, 2)[None, :]
    for c in (1, 2):
        p = _pad_edge(ycc[..., c], 2 * rows, 2 * cw)
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(_pad_edge(d, up8(rows), cw))
    return out


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """jfdctint.c on (..., 8, 8) samples - 128 (rows, then columns); int64 here,
    every intermediate fits int32."""
    C = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137,
             f1961=16069, f2053=16819, f2562=20995, f3072=25172)

    def pass_(d, first):
        d = [d[..., i] for i in range(8)]
        t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
        t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        n = 11 if first else 15
        ds = lambda x, s: (x + (1 << (s - 1))) >> s
        o = [None] * 8
        if first:
            o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
        else:
            o[0], o[4] = ds(t10 + t11, 2), ds(t10 - t11, 2)
        z1 = (t12 + t13) * C["f0541"]
        o[2] = ds(z1 + t13 * C["f0765"], n)
        o[6] = ds(z1 - t12 * C["f1847"], n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * C["f1175"]
        t4, t5, t6, t7 = t4 * C["f0298"], t5 * C["f2053"], t6 * C["f3072"], t7 * C["f1501"]
        z1, z2, z3, z4 = -z1 * C["f0899"], -z2 * C["f2562"], -z3 * C["f1961"] + z5, -z4 * C["f0390"] + z5
        o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, n), ds(t5 + z2 + z4, n), ds(t6 + z2 + z3, n), ds(t7 + z1 + z4, n)
        return np.stack(o, axis=-1)

    x = pass_(blocks.astype(np.int64), True)                 # along each row
    return np.swapaxes(pass_(np.swapaxes(x, -1, -2), False), -1, -2)   # along each column


def quantise(coef: np.ndarray, table: np.ndarray) -> np.ndarray:
    """coef / (8·q), halves away from zero; (..., 8, 8) with a natural-order table."""
    d = 8 * table.reshape(8, 8)
    return np.sign(coef) * ((np.abs(coef) + d // 2) // d)


def plane_blocks(plane: np.ndarray, table: np.ndarray) -> np.ndarray:
    """(rows, cols, 64) quantised coefficients in zigzag order of a component's blocks."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(hb, 8, wb, 8).swapaxes(1, 2) - 128
    return quantise(fdct_islow(b), table).reshape(hb, wb, 64)[..., ZIGZAG]


@dataclass
class Counters:
    zrl: int = 0            # 0xF0 codes
    no_eob: int = 0         # blocks whose coefficient 63 is not zero
    stuffed: int = 0        # 0xFF bytes of the entropy data (each followed by 0x00)
    dummy: int = 0          # blocks beyond a component's ⌈size / 8⌉ grid
    max_dc_cat: int = 0
    max_ac_cat: int = 0
    blocks: int = 0


def scan_blocks(a: np.ndarray, quality: int, subsampling: str):
    """The scan's blocks in order: a list of (component, zigzag coefficients,
    is_dummy).  A dummy block has zero AC terms and the DC of the block before
    it in the MCU."""
    h, w = a.shape[:2]
    tabs = quant_tables(quality)
    planes = component_planes(a, subsampling)
    coefs = [plane_blocks(p, tabs[0 if c == 0 else 1]) for c, p in enumerate(planes)]
    out = []
    if subsampling == "4:4:4":
        for my in range(coefs[0].shape[0]):
            for mx in range(coefs[0].shape[1]):
                out += [(c, coefs[c][my, mx], False) for c in range(3)]
        return out
    hb, wb = coefs[0].shape[:2]
    for my in range((h + 15) // 16):
        for mx in range((w + 15) // 16):
            prev = None
            for j in range(4):
                by, bx = 2 * my + (j >> 1), 2 * mx + (j & 1)
                if by < hb and bx < wb:
                    prev = coefs[0][by, bx]
                    out.append((0, prev, False))
                else:
                    z = np.zeros(64, np.int64)
                    z[0] = prev[0]
                    prev = z
                    out.append((0, z, True))
            out += [(c, coefs[c][my, mx], False) for c in (1, 2)]
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, ln):
        self.acc = (self.acc << ln) | code
        self.n += ln
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def finish(self) -> bytes:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _cat(v: int) -> int:
    return int(abs(v)).bit_length()


def entropy_unstuffed(blocks, ctr: Counters) -> bytes:
    """Huffman-coded bits of the scan, MSB first, the last byte filled with
    1-bits; not yet byte-stuffed."""
    dc_t = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
    ac_t = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
    bw, last = _Bits(), [0, 0, 0]
    for comp, zz, dummy in blocks:
        t = 0 if comp == 0 else 1
        ctr.blocks += 1
        ctr.dummy += bool(dummy)
        dc = int(zz[0])
        diff, last[comp] = dc - last[comp], dc
        n = _cat(diff)
        ctr.max_dc_cat = max(ctr.max_dc_cat, n)
        bw.put(*dc_t[t][n])
        if n:
            bw.put((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)
        run = 0
        for k in range(1, 64):
            v = int(zz[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                bw.put(*ac_t[t][0xF0])
                ctr.zrl += 1
                run -= 16
            n = _cat(v)
            ctr.max_ac_cat = max(ctr.max_ac_cat, n)
            bw.put(*ac_t[t][(run << 4) | n])
            bw.put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)
            run = 0
        if run:
            bw.put(*ac_t[t][0x00])
        else:
            ctr.no_eob += 1
    return bw.finish()


def entropy(a: np.ndarray, quality: int = 75, subsampling: str = "4:2:0") -> Tuple[bytes, Counters]:
    """The byte-stuffed entropy data (what ipp_jpeg_encode leaves in a slot)."""
    assert subsampling in SAMPLINGS and a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8
    ctr = Counters()
    raw = entropy_unstuffed(scan_blocks(a, quality, subsampling), ctr)
    ctr.stuffed = raw.count(0xFF)
    return raw.replace(b"\xff", b"\xff\x00"), ctr


def encode(a: np.ndarray, quality: int = 75, subsampling: str = "4:2:0") -> Tuple[bytes, Counters]:
    """The whole file: header, stuffed entropy data, EOI; and the counters."""
    body, ctr = entropy(a, quality, subsampling)
    return header(a.shape[1], a.shape[0], quality, subsampling) + body + b"\xff\xd9", ctr


def pillow_subsampling(subsampling: str) -> int:
    return {"4:4:4": 0, "4:2:0": 2}[subsampling]


# ---- inputs shared by the CPU and GPU tests ---------------------------------
QUALITIES = (1, 10, 25, 50, 75, 90, 95, 100)


def noise(h: int, w: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), np.uint8)


def constant(h: int, w: int, rgb=(200, 30, 90)) -> np.ndarray:
    return np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)).copy()


def ramps(h: int, w: int) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 7) % 256],
                    axis=-1).astype(np.uint8)


def primaries(h: int, w: int) -> np.ndarray:
    """Saturated primaries and their complements in 5 x 3 px cells: hard edges
    at every phase of the block and chroma grids."""
    cols = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
                     (0, 0, 0), (255, 255, 255)], np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return cols[((xx // 5) * 3 + (yy // 3) * 5) % 8]


def mixed(h: int, w: int, seed: int = 3) -> np.ndarray:
    """Every coding path in one image: noise (blocks without EOB, 0xFF bytes),
    a dark ramp with sparse bright pixels (long zero runs before a late
    coefficient: ZRL), flat areas (EOB at once) and a hard-edged stripe."""
    rng = np.random.default_rng(seed)
    a = ramps(h, w) // 3
    a[: max(h // 2, 1), : max(w // 2, 1)] = rng.integers(0, 256, (max(h // 2, 1), max(w // 2, 1), 3), np.uint8)
    salt = rng.random((h, w)) < 0.02
    salt[: h // 2, : w // 2] = False
    a[salt] = 255
    a[:, (3 * w) // 4:(3 * w) // 4 + 3] = (255, 0, 255)
    return a


CONTENTS = dict(noise=noise, constant=constant, ramps=ramps, primaries=primaries, mixed=mixed)
