"""CPU-side readers of the pipe's MFMA tap tiles, written in plain numpy from
the description in csrc/ipp_pipe_layout.h (no library call decodes anything
here): the tests of the host tile builder ipp_plan_mfma_tile decode its tiles
with these and compare with Pillow's taps."""
import numpy as np

from image_processor_pipeline_amd import _native as N


def tap_axis(n_in, n_out, identity=0, shift=0, phase=0, compact=0):
    """A TAP_AXIS record [1] as the planner fills it (coef_off 0)."""
    lib = N.load()
    a = np.zeros(1, N.TAP_AXIS)
    ks = 1 if identity else lib.ipp_plan_lanczos_ksize(0.0, float(n_in), n_out)
    a["in_size"], a["out_size"], a["identity"], a["shift"], a["phase"] = n_in, n_out, identity, shift, phase
    a["nkb"], a["compact"] = lib.ipp_plan_mfma_nk_bound(n_in, n_out, ks), compact
    a["n_tiles"] = (n_out + phase + 15) // 16
    return a


def tile_operand(h4, blk):
    """The B operand of every K step of one tile: int64 [plane 3][K step nK][k 64][col 16], the balanced byte
    `plane` of output col's tap at input K0 + 64·s + k.

    Dense (h4[3] = 0): block (s, p) is 64 lanes × 16 B at uint4 (3s + p)·64; lane l, byte j = output l & 15 at
    k = 16·(l >> 4) + j.  Compact (h4[3] = 1): 4 uint4 of meta, meta[n] = g0 | len << 8 | base << 16 of output n;
    then plane p's 16-column group blocks at uint4 4 + 64p + i, block base + j = output n's group g0 + j counted
    from K0; everything else is zero."""
    nk = int(h4[1])
    b = blk[:nk * 3072].view(np.int8).astype(np.int64)
    if not h4[3]:
        return b.reshape(nk, 3, 4, 16, 16).transpose(1, 0, 2, 4, 3).reshape(3, nk, 64, 16)
    assert nk >= 2
    meta = blk[:64].view(np.int32)
    groups = b.reshape(-1, 16)                # uint4 blocks
    out = np.zeros((3, nk * 64, 16), np.int64)
    used = np.zeros(len(groups), bool)
    used[:4] = True
    nb = 0
    for n in range(16):
        g0, ln, base = int(meta[n]) & 255, int(meta[n]) >> 8 & 255, int(meta[n]) >> 16
        assert base == nb and 16 * (g0 + ln) <= 64 * nk
        nb += ln
        for p in range(3):
            out[p, 16 * g0:16 * (g0 + ln), n] = groups[4 + 64 * p + base:4 + 64 * p + base + ln].reshape(-1)
            used[4 + 64 * p + base:4 + 64 * p + base + ln] = True
    assert nb <= 64 and not groups[~used].any()
    return out.reshape(3, nk, 64, 16)


def tile_taps(h4, blk):
    """int64 [64·nK][16]: the tap of output col at input K0 + x, the balanced bytes recombined."""
    B = tile_operand(h4, blk).reshape(3, -1, 16)
    return B[0] + 256 * B[1] + 65536 * B[2]
