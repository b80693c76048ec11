"""CPU restatement of the decoder include/ipp.h states under ipp_jpeg_decode:
plain Python for the marker walk's consumer and the Huffman decode (from the
file's own tables), NumPy for the per-sample arithmetic.  No Pillow call here:
the tests compare `decode` with Image.open(f).convert("RGB")."""
from __future__ import annotations

import numpy as np

from tests.jpeg_refs import ZIGZAG


def _codes(bits, vals):
    """(length, code) -> symbol of a (BITS, HUFFVAL) table (Annex C)."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[(ln, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    """MSB-first reader of one restart interval; a 0x00 after 0xFF is no data."""

    def __init__(self, data: bytes):
        self.d = data.replace(b"\xff\x00", b"\xff")
        self.p = 0

    def bit(self) -> int:
        if self.p >= 8 * len(self.d):
            raise ValueError("the interval ends early")
        b = (self.d[self.p >> 3] >> (7 - (self.p & 7))) & 1
        self.p += 1
        return b

    def bits(self, n: int) -> int:
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table) -> int:
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | self.bit()
            if (ln, code) in table:
                return table[(ln, code)]
        raise ValueError("a code in no table")


def _extend(v: int, s: int) -> int:
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def coefficients(data: bytes, info) -> np.ndarray:
    """(blocks in scan order, 64) quantised coefficients, natural order."""
    s420 = info.subsampling == "4:2:0"
    side, comps = (16, (0, 0, 0, 0, 1, 2)) if s420 else (8, (0, 1, 2))
    nmcu = ((info.w + side - 1) // side) * ((info.h + side - 1) // side)
    dc_t = [_codes(*info.htables[(0, t)]) for t in info.dc]
    ac_t = [_codes(*info.htables[(1, t)]) for t in info.ac]
    span = data[info.span[0]:info.span[1]]
    ri = info.restart_interval if 0 < info.restart_interval < nmcu else nmcu
    segs, at, k = [], 0, 0
    while True:
        j = at
        while True:
            j = span.find(b"\xff", j)
            if j < 0 or j + 1 >= len(span) or 0xD0 <= span[j + 1] <= 0xD7:
                break
            j += 2
        if j < 0 or j + 1 >= len(span):
            segs.append(span[at:])
            break
        if span[j + 1] - 0xD0 != k % 8:
            raise ValueError("RSTn out of order")
        segs.append(span[at:j])
        at, k = j + 2, k + 1
    if len(segs) != (nmcu + ri - 1) // ri:
        raise ValueError("the wrong number of restart intervals")
    out = np.zeros((nmcu * len(comps), 64), np.int64)
    for s, seg in enumerate(segs):
        br, pred = _Bits(seg), [0, 0, 0]
        for m in range(s * ri, min((s + 1) * ri, nmcu)):
            for j, c in enumerate(comps):
                blk = out[m * len(comps) + j]
                t = br.symbol(dc_t[c])
                if t > 11:
                    raise ValueError("a DC category baseline does not have")
                pred[c] += _extend(br.bits(t), t)
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs = br.symbol(ac_t[c])
                    r, t = rs >> 4, rs & 15
                    if t == 0:
                        if r == 15:
                            k += 16
                            if k > 63:
                                raise ValueError("a run past coefficient 63")
                            continue
                        if r:
                            raise ValueError("an EOB run baseline does not have")
                        break
                    k += r
                    if k > 63 or t > 10:
                        raise ValueError("a run past coefficient 63")
                    blk[ZIGZAG[k]] = _extend(br.bits(t), t)
                    k += 1
        if 8 * len(br.d) - br.p >= 8:
            raise ValueError("bytes left over in the interval")
    return out


def _idct_pass(c, s):
    c = [c[..., i] for i in range(8)]
    z1 = (c[2] + c[6]) * 4433
    t2, t3 = z1 - c[6] * 15137, z1 + c[2] * 6270
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([(x + (1 << (s - 1))) >> s for x in o], axis=-1)


def samples(coef: np.ndarray, table: np.ndarray) -> np.ndarray:
    """(..., 8, 8) samples 0..255 of (..., 64) coefficients: dequantise, the
    islow inverse transform (columns, then rows), + 128, clamp."""
    x = (coef * table.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    x = np.swapaxes(_idct_pass(np.swapaxes(x, -1, -2), 11), -1, -2)   # along each column
    return np.clip(_idct_pass(x, 18) + 128, 0, 255)                   # along each row


def upsample_h2v2(p: np.ndarray, w: int, h: int) -> np.ndarray:
    """jdsample.c for a chroma plane of its real extent ⌈w/2⌉ x ⌈h/2⌉."""
    ch, cw = p.shape
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w]
    y = np.arange(h)
    near = y >> 1
    far = np.clip(np.where(y % 2 == 0, near - 1, near + 1), 0, ch - 1)
    s = 3 * p[near] + p[far]
    sp = np.pad(s, ((0, 0), (1, 1)), mode="edge")
    out = np.zeros((h, 2 * cw), np.int64)
    out[:, 0::2] = (3 * s + sp[:, :-2] + 8) >> 4
    out[:, 1::2] = (3 * s + sp[:, 2:] + 7) >> 4
    return out[:, :w]


def decode(data: bytes, info) -> np.ndarray:
    """(h, w, 3) uint8 RGB of a file parse_jpeg accepted (info)."""
    w, h = info.w, info.h
    s420 = info.subsampling == "4:2:0"
    side, bpm = (16, 6) if s420 else (8, 3)
    mx, my = (w + side - 1) // side, (h + side - 1) // side
    coef = coefficients(data, info).reshape(my, mx, bpm, 64)
    q = [info.qtables[t] for t in info.qt]

    def plane(blocks):     # (rows, cols, 8, 8) -> (8 rows, 8 cols)
        return blocks.swapaxes(1, 2).reshape(blocks.shape[0] * 8, blocks.shape[1] * 8)
    if s420:
        ys = samples(coef[:, :, :4], q[0]).reshape(my, mx, 2, 2, 8, 8)
        Y = ys.transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16)[:h, :w]
        cb, cr = (upsample_h2v2(plane(samples(coef[:, :, 3 + c], q[c]))[:(h + 1) // 2, :(w + 1) // 2], w, h)
                  for c in (1, 2))
    else:
        Y, cb, cr = (plane(samples(coef[:, :, c], q[c]))[:h, :w] for c in range(3))
    cb, cr = cb - 128, cr - 128
    rgb = [Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
           Y + ((116130 * cb + 32768) >> 16)]
    return np.clip(np.stack(rgb, axis=-1), 0, 255).astype(np.uint8)
