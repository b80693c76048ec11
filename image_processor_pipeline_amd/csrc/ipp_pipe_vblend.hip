// ipp_pipe_vblend.hip — the V launch of the fused 5-stage pipe: the LANCZOS
// vertical pass over T (the H launch's output, ipp_pipe.hip) on the matrix
// cores (v_mfma_i32_16x16x64_i8), fused with unpremultiply and the alpha
// blend onto the background (overlays.py:129,138-139).  It visits the
// overlay's 16-row bands alone: the H launch's copy blocks wrote the rest of
// the composite.  The exact integer arithmetic (balanced tap bytes, pixels
// XOR 0x80) is stated in ipp_pipe.hip's header, the tap tiles, T and the
// bands in ipp_pipe_layout.h.
//
// V pass on MFMA (tap tiles aligned with 16-row background bands: the plan's
// phase = p.y mod 16) → unpremultiply → blend onto the background.  Block =
// 16 composite rows of one item.  A = taps of the band's 16 overlay rows (lane
// l: row l&15, T rows 16(l>>4)..+15 of the K step), B = 64 T rows × 16
// overlay columns of one channel (four 16-B T groups per lane give all four
// channels), D lane l = column l&15, rows 4(l>>4)..+3.
//
// Horner accumulation over the tap byte planes (round 6): one accumulator per
// channel instead of one per (channel, plane) — plane 2's products summed over
// every K step, shifted left by 8, plane 1's added, shifted again with the row
// bias added (v_lshl_add), then plane 0's: ((S2 << 8) + S1) << 8 + bias + S0
// equals planes3(bias + S0, S1, S2) in int32 wrap-around arithmetic.  It
// frees 32 VGPRs of the 48 the accumulators took.
//
// Experiment switches left in this file are the live ones that DESIGN.md §3
// names (IPP_VB_WPE/DB/HOIST_MAX).
#include <algorithm>
#include <type_traits>

#include "ipp_device.h"
#include "ipp_pipe_layout.h"

namespace {

using namespace pipe_layout;

// V pass: column tiles with nK ≤ IPP_VB_DB double-buffer their T groups (the
// wave's next tile's loads fly during this tile's MFMAs).
#ifndef IPP_VB_DB
#define IPP_VB_DB 2
#endif
// V pass: the band's taps loaded once for all its column tiles (nK ≤
// IPP_VB_HOIST_MAX; larger nK load each K step's taps per column tile).  Of
// the bench's V tiles 7 % have nK 1, 74 % nK 2, 19 % nK 3.
#ifndef IPP_VB_HOIST_MAX
#define IPP_VB_HOIST_MAX 3
#endif
// V pass occupancy target (waves per SIMD).  Round 5 (three accumulators per
// channel): 3 fit 160 VGPRs with every nK ≤ 4 hoisted (the compiler's own
// choice, 168 VGPRs + 52 AGPRs, gave 2 waves): 1.49-1.52 -> 1.37-1.40 ms.
#ifndef IPP_VB_WPE
#define IPP_VB_WPE 3
#endif

// orow (the band's unpremultiplied overlay rows in LDS) is indexed by
// composite column - (p.x & ~15), so a 16-pixel composite group reads its 16
// overlay pixels with four aligned ds_read_b128; the ≤ 15 columns before the
// overlay and after it are zero (α 0: the background stays).
__host__ __device__ constexpr int orow_stride(int ov_w_max) { return (ov_w_max + 32 + 3) & ~3; }
// The widest overlay the V launch takes: its rows must fit 64 KB of LDS
// (IPP_PIPE_MAX_OV_W in ipp.h; the magic-divisor table is dropped for
// overlays too wide to hold it beside the rows).
static_assert((size_t)kBandRows * orow_stride(IPP_PIPE_MAX_OV_W) * 4 <= 64 * 1024, "V-pass rows in LDS");
static_assert((size_t)kBandRows * orow_stride(IPP_PIPE_MAX_OV_W + 1) * 4 > 64 * 1024, "IPP_PIPE_MAX_OV_W is the limit");

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// Paste.c BLEND on two bytes at once (16-bit lanes): DIV255(bg·(255 - a) +
// ov·a), written as 255·bg + 128 + (ov - bg)·a (mod 2^16: the true value is
// in [0, 65153]) followed by DIV255's (t + (t >> 8)) >> 8.
__device__ __forceinline__ uint32_t blend_u16x2(uint32_t bg, uint32_t ov, uint32_t al) {
    const u16x2 b = __builtin_bit_cast(u16x2, bg), o = __builtin_bit_cast(u16x2, ov), a = __builtin_bit_cast(u16x2, al);
    const u16x2 c255 = {255, 255}, c128 = {128, 128}, c8 = {8, 8};
    const u16x2 t = (u16x2)(o - b) * a + (b * c255 + c128);
    return __builtin_bit_cast(uint32_t, (u16x2)((u16x2)(t + (t >> c8)) >> c8));
}

// 16 composite pixels (48 bytes, bg[0..11]) blended in place with 16 RGBA
// overlay pixels (ov[0..15]).  Byte j of the row segment is channel j mod 3
// of pixel j / 3; each output dword is done as two byte pairs (bytes 0, 2 and
// 1, 3) in 16-bit lanes, the overlay byte and its pixel's α gathered by v_perm.
__device__ __forceinline__ void blend48(uint32_t (&bg)[12], const uint32_t (&ov)[16]) {
#pragma unroll
    for (int d = 0; d < 12; ++d) {
        uint32_t r[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j0 = 4 * d + h, j1 = j0 + 2;                 // the pair's bytes
            const int p0 = j0 / 3, p1 = j1 / 3, c0 = j0 % 3, c1 = j1 % 3;
            // v_perm(hi, lo, sel): bytes 0-3 of lo = sel 0-3, of hi = 4-7; 0x0c = 0
            const uint32_t sel_ov = (uint32_t)c0 | 0x0c00u | ((uint32_t)(p1 == p0 ? c1 : 4 + c1) << 16) | 0x0c000000u;
            const uint32_t sel_al = 3u | 0x0c00u | ((uint32_t)(p1 == p0 ? 3 : 7) << 16) | 0x0c000000u;
            const uint32_t ovp = __builtin_amdgcn_perm(ov[p1], ov[p0], sel_ov);
            const uint32_t alp = __builtin_amdgcn_perm(ov[p1], ov[p0], sel_al);
            const uint32_t bgp = __builtin_amdgcn_perm(0u, bg[d], h ? 0x0c030c01u : 0x0c020c00u);
            r[h] = blend_u16x2(bgp, ovp, alp);
        }
        bg[d] = __builtin_amdgcn_perm(r[1], r[0], 0x06020400u);  // r0 b0, r1 b0, r0 b2, r1 b2
    }
}

// acc = (acc << 8) + (a0, a1, a2, a3) (Horner step; the compiler emits one
// v_lshl_add_u32 per dword.  Plain code, not inline asm: the MFMA results it
// reads need the wait states the compiler's hazard recognizer inserts, which
// it does not do for an asm operand.)
__device__ __forceinline__ void horner8(i32x4& acc, int32_t a0, int32_t a1, int32_t a2, int32_t a3) {
    acc = (acc << 8) + i32x4{a0, a1, a2, a3};
}

// Channel c's B operand of one K step: dword c of its four T groups (a
// register transpose the MFMA needs anyway: its source tuple must be four
// consecutive registers).
__device__ __forceinline__ i32x4 vb_bop(const u32x4_t (&g)[4], int c) {
    return i32x4{(int)g[0][c], (int)g[1][c], (int)g[2][c], (int)g[3][c]};
}

// One column tile's V sums, Horner over the tap byte planes (see above):
// plane 2's MFMAs over all NK K steps, << 8, plane 1's, << 8 with the row
// biases, plane 0's.  bq = the channel-major B operands (vb_bop) per K step.
template <int NK>
__device__ __forceinline__ void vb_mfma_tile(const i32x4 (&ta)[NK][3], const i32x4 (&bq)[NK][4], const int32_t (&rb)[4],
                                             i32x4 (&acc)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int q = 2; q >= 0; --q) {
#pragma unroll
        for (int ks = 0; ks < NK; ++ks)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ta[ks][q], bq[ks][c], acc[c], 0, 0, 0);
        if (q == 2) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] <<= 8;
        } else if (q == 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) horner8(acc[c], rb[0], rb[1], rb[2], rb[3]);
        }
    }
}

// One V-pass block: band ty of item im, counted from the first 16-row band
// the overlay touches (the rows outside those bands: ipp_pipe_hpass_bgcopy).
// MAGIC: unpremultiply by the per-block LDS table of magic divisors (exact,
// unpremultiply_magic) instead of a reciprocal and two fix-ups per channel:
// 1.340 -> 1.319 ms (round 5, profiles/r05/vpass/ab_unpremul_magic_r05al.txt);
// overlays too wide for the table beside their rows take the reciprocal.
//
// INPLACE (ipp_pipe_vblend_over, a later layer of a scene): bg and dst are the
// same pointer — the composite the earlier layers left — and are therefore
// not __restrict__; the descriptor's bg_off / bg_pitch are replaced by its
// dst_off / dst_pitch.  Why the block may blend in place:
//   * phase 1 reads tmp and coefs and writes LDS only;
//   * phase 2 walks a set of disjoint byte ranges of the band's rows — the
//     48-byte groups (grouped path), the 16-byte chunks (general path) — and
//     each range belongs to exactly one thread of the block, which loads it
//     (gload / load16) before it stores it and never touches it again: the
//     prefetch of the thread's next range (gnxt, the four chunks in flight)
//     is another range, owned by the same thread.  No thread reads a byte
//     another thread of the launch writes, so neither a barrier nor any order
//     among blocks is needed;
//   * the blocks of one descriptor own disjoint 16-row bands, and two
//     descriptors of one launch never share a composite (the caller's
//     contract, ipp.h);
//   * a range's bytes outside the overlay's rectangle are stored as loaded:
//     not blended (rows outside [oy_lo, oy_hi), groups or chunks beside the
//     overlay) or blended with the zero alpha of orow's margin columns, and
//     BLEND(b, ·, 0) = DIV255(255 b + 128) = b.
// Under the column split it visits the overlay's groups [sx0, sx1) alone;
// otherwise the band rows.
template <bool INPLACE>
struct VbPtr {
    typedef const uint8_t* __restrict__ bg_t;
    typedef uint8_t* __restrict__ dst_t;
};
template <>
struct VbPtr<true> {
    typedef const uint8_t* bg_t;
    typedef uint8_t* dst_t;
};
__device__ __forceinline__ ipp_paste_desc vb_paste_desc(const ipp_paste_desc& q, bool inplace) {
    ipp_paste_desc p = q;
    if (inplace) {
        p.bg_off = p.dst_off;
        p.bg_pitch = p.dst_pitch;
    }
    return p;
}

template <bool MAGIC, bool INPLACE = false>
__device__ __forceinline__ void vblend_block(uint32_t* __restrict__ orow, const uint8_t* __restrict__ tmp,
                                             typename VbPtr<INPLACE>::bg_t bg, typename VbPtr<INPLACE>::dst_t dst,
                                             const int32_t* __restrict__ coefs,
                                             const ipp_pipe_desc* __restrict__ descs, int im, int ty, int ov_w_max,
                                             const uint16_t* __restrict__ trim) {
    const ipp_paste_desc p = vb_paste_desc(descs[im].p, INPLACE);
    int y0 = ty * kBandRows;
    {
        int vb0, vb1;
        paste_bands(p, vb0, vb1);
        y0 += vb0;
        if (y0 >= vb1) return;
    }
    if (y0 >= p.bg_h) return;
    const int nrows = min(kBandRows, p.bg_h - y0);
    const int oy_lo = max(0, y0 - p.y), oy_hi = min(p.ov_h, y0 + nrows - p.y);
    const bool any = oy_lo < oy_hi;  // block-uniform
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    const int os = orow_stride(ov_w_max), xo = p.x & 15;  // orow column of overlay column 0
    const uint8_t* bgb = bg + p.bg_off + (int64_t)y0 * p.bg_pitch;
    uint8_t* dsb = dst + p.dst_off + (int64_t)y0 * p.dst_pitch;
    const bool groups = (p.bg_w & 15) == 0 && ((p.bg_pitch | p.dst_pitch) & 15) == 0 &&
                        ((reinterpret_cast<uintptr_t>(bgb) | reinterpret_cast<uintptr_t>(dsb)) & 15u) == 0;
    // groups per row visited: all of them, or (column split) the overlay's
    // [sx0, sx1) — the H pass's copy blocks wrote the rest of the band rows
    int sx0, sx1;
    const bool csplit = groups && band_cols_split(p, bg, dst, sx0, sx1);
    const int gc0 = csplit ? sx0 : 0;
    const int G = csplit ? sx1 - sx0 : p.bg_w >> 4, lg = 31 - __builtin_clz(max(G, 1));
    const bool pow2 = (G & (G - 1)) == 0;
    const int gtotal = nrows * G;
    auto gload = [&](int idx, uint4 (&v)[3]) {
        const int rr = pow2 ? idx >> lg : idx / G;
        const int gi = gc0 + idx - rr * G;
        const uint4* sp = reinterpret_cast<const uint4*>(bgb + (int64_t)rr * p.bg_pitch) + 3 * gi;
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] = sp[q];
    };
    uint4 gcur[3];
    if (any) {
        uint32_t* umag = orow + kBandRows * os;  // MAGIC: the unpremultiply divisors
        if (MAGIC) {
            umag[threadIdx.x] = unpremul_magic(threadIdx.x);
            __syncthreads();
        }
        // zero the ≤ 15 columns before the overlay and the 16 after it
        for (int e = threadIdx.x; e < kBandRows * 32; e += 256) {
            const int row = e >> 5, c = e & 31;
            if (c < xo) orow[row * os + c] = 0u;
            else if (c >= 16) orow[row * os + xo + p.ov_w + c - 16] = 0u;
        }
        const ipp_resample_desc v = descs[im].v;
        const int phase = tap_phase(p.y);
        const int t = band_tap_tile(y0, p.y, phase);
        const TapTiles tt = tap_tiles(coefs, v.coef_off, tap_ntiles(v.out_len, phase));
        const int4 th = tt.hdr[t];
        const int ctiles = (p.ov_w + 15) >> 4;
        const int gstride = t_pitch_vecs(v.src_pitch);
        const int x_l = lane & 15;
        // the row biases (added at the last Horner step)
        int32_t rb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) rb[r] = tt.bias[kBiasWords * t + 4 * (lane >> 4) + r];
        const u32x4_t* tbase = reinterpret_cast<const u32x4_t*>(tmp + v.src_off);
        const int gbase = t_row_group(th.x + 16 * (lane >> 4));
        // The trim entry of the lane's H band of K step ks (trim = the item's
        // row of the H launch's trim table, ipp_pipe_layout.h): the band does
        // not depend on the column tile, so a block reads its entries once.
        // No table: nothing is constant.
        const int hbands = trim_bands(descs[im].h.lines);
        auto tentry = [&](int ks) -> uint32_t {
            if (!trim) return kTrimNone;
            const int hb = trim_v_band(th.x, ks, lane);
            return hb < hbands ? (uint32_t)trim[hb] : kTrimAll;
        };
        // T groups of K step ks of column tile ct: rows th.x + 64 ks + 16 (lane >> 4) .. + 15,
        // one H band (entry e): loaded, or 0x80 in every byte where the H launch left them unstored
        auto tload = [&](int ct, int ks, uint32_t e, u32x4_t (&g)[4]) {
            if (trim_const(e, ct)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = u32x4_t{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
            } else {
                const int xs = min(16 * ct + x_l, p.ov_w - 1);
                const u32x4_t* tq = t_group(tbase, gstride, gbase + kKStepGroups * ks, xs);
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = tq[j * gstride];
            }
        };
        // the tile's unpremultiplied overlay pixels into the band's LDS rows
        // (s(c, r) = the sum of channel c, tile row r)
        auto epilogue = [&](int ct, auto s) {
            const int x = 16 * ct + x_l;
            if (x < p.ov_w) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * (lane >> 4) + r;  // band row = tile row
                    const int o = y0 + row - p.y;         // overlay row
                    if (o >= oy_lo && o < oy_hi) {
                        const uint32_t px = clip8x4_mfma(s(0, r), s(1, r), s(2, r), s(3, r));
                        orow[row * os + xo + x] = MAGIC ? unpremultiply_magic(px, umag) : unpremultiply(px);
                    }
                }
            }
        };
        // The band's taps (the A operand) are the same for every column tile:
        // with nK ≤ IPP_VB_HOIST_MAX they are loaded once, before the column
        // tiles, and every tile's T groups for all its K steps are issued
        // before its MFMAs.
        auto tiles = [&](auto nkc) {
            constexpr int NK = decltype(nkc)::value;
            if constexpr (NK > 0) {
                i32x4 ta[NK][3];
#pragma unroll
                for (int ks = 0; ks < NK; ++ks)
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        ta[ks][q] = __builtin_bit_cast(i32x4, tt.blk[th.z + tap_dense_block(ks, q, lane)]);
                // the lane's trim entries, K step ks in bits 16 ks .. 16 ks + 15
                static_assert(NK <= 4, "four 16-bit trim entries in 64 bits");
                uint64_t tpk = 0;
#pragma unroll
                for (int ks = 0; ks < NK; ++ks) tpk |= (uint64_t)tentry(ks) << (16 * ks);
                auto te = [&](int ks) { return (uint32_t)(tpk >> (16 * ks)) & 0xFFFFu; };
                // the loaded T groups of a tile, turned channel-major
                auto transpose = [&](const u32x4_t (&g)[NK][4], i32x4 (&bq)[NK][4]) {
#pragma unroll
                    for (int ks = 0; ks < NK; ++ks)
#pragma unroll
                        for (int c = 0; c < 4; ++c) bq[ks][c] = vb_bop(g[ks], c);
                };
                if constexpr (NK <= IPP_VB_DB) {
                    // double-buffered T groups: the wave's next column tile's
                    // loads are in flight during this tile's MFMAs and
                    // epilogue; the buffer carried to the next tile is the
                    // channel-major operands, so raw and transposed groups
                    // are never live together
                    i32x4 bc[NK][4];
                    u32x4_t gn[NK][4];
                    int ct = wave;
                    if (ct < ctiles) {
#pragma unroll
                        for (int ks = 0; ks < NK; ++ks) tload(ct, ks, te(ks), gn[ks]);
                        transpose(gn, bc);
                    }
                    for (; ct < ctiles; ct += 4) {
                        const bool more = ct + 4 < ctiles;
                        if (more) {
#pragma unroll
                            for (int ks = 0; ks < NK; ++ks) tload(ct + 4, ks, te(ks), gn[ks]);
                        }
                        i32x4 acc[4];
                        vb_mfma_tile<NK>(ta, bc, rb, acc);
                        epilogue(ct, [&](int c, int r) { return acc[c][r]; });
                        if (more) transpose(gn, bc);
                    }
                } else {
                    for (int ct = wave; ct < ctiles; ct += 4) {
                        u32x4_t g[NK][4];
#pragma unroll
                        for (int ks = 0; ks < NK; ++ks) tload(ct, ks, te(ks), g[ks]);
                        i32x4 bq[NK][4];
                        transpose(g, bq);
                        i32x4 acc[4];
                        vb_mfma_tile<NK>(ta, bq, rb, acc);
                        epilogue(ct, [&](int c, int r) { return acc[c][r]; });
                    }
                }
            } else {
                // nK beyond the hoisted forms: each K step's taps and T groups
                // loaded in turn, one accumulator per (channel, plane) (and the
                // K step's trim entry: nK has no bound here to keep them all)
                for (int ct = wave; ct < ctiles; ct += 4) {
                    i32x4 acc[4][3];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        acc[c][0] = i32x4{rb[0], rb[1], rb[2], rb[3]};
                        acc[c][1] = i32x4{0, 0, 0, 0};
                        acc[c][2] = i32x4{0, 0, 0, 0};
                    }
#pragma unroll 1
                    for (int ks = 0; ks < th.y; ++ks) {
                        i32x4 a[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) a[q] = __builtin_bit_cast(i32x4, tt.blk[th.z + tap_dense_block(ks, q, lane)]);
                        u32x4_t g[4];
                        tload(ct, ks, tentry(ks), g);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const i32x4 bq = vb_bop(g, c);
#pragma unroll
                            for (int q = 0; q < 3; ++q)
                                acc[c][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[q], bq, acc[c][q], 0, 0, 0);
                        }
                    }
                    epilogue(ct, [&](int c, int r) { return planes3(acc[c][0][r], acc[c][1][r], acc[c][2][r]); });
                }
            }
        };
        // (a tile with more K steps than IPP_VB_HOIST_MAX takes the generic loop)
        switch (th.y <= IPP_VB_HOIST_MAX ? th.y : 0) {
            case 1: tiles(std::integral_constant<int, 1>{}); break;
#if IPP_VB_HOIST_MAX >= 2
            case 2: tiles(std::integral_constant<int, 2>{}); break;
#endif
#if IPP_VB_HOIST_MAX >= 3
            case 3: tiles(std::integral_constant<int, 3>{}); break;
#endif
#if IPP_VB_HOIST_MAX >= 4
            case 4: tiles(std::integral_constant<int, 4>{}); break;
#endif
            default: tiles(std::integral_constant<int, 0>{}); break;
        }
        __syncthreads();
    }

    // Phase 2: composite rows = background bytes, blended inside the footprint.
    const int row_bytes = 3 * p.bg_w;
    if (groups) {
        // 16-pixel groups: 48 bytes per thread and step (three 16-B loads in
        // flight; the next step's loads are issued before this step's blend
        // and stores), the overlay pixels from orow, blended in 16-bit lanes.
        const int gx0 = p.x >> 4, gx1 = (p.x + p.ov_w + 15) >> 4;  // groups the overlay touches
        if ((int)threadIdx.x < gtotal) gload(threadIdx.x, gcur);
        for (int idx = threadIdx.x; idx < gtotal; idx += 256) {
            uint4 gnxt[3];
            if (idx + 256 < gtotal) gload(idx + 256, gnxt);
            const int rr = pow2 ? idx >> lg : idx / G;
            const int gi = gc0 + idx - rr * G;
            uint32_t w[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                w[4 * q] = gcur[q].x;
                w[4 * q + 1] = gcur[q].y;
                w[4 * q + 2] = gcur[q].z;
                w[4 * q + 3] = gcur[q].w;
            }
            const int o = y0 + rr - p.y;
            if (any && o >= oy_lo && o < oy_hi && gi >= gx0 && gi < gx1) {
                const uint4* orw = reinterpret_cast<const uint4*>(orow + rr * os + 16 * (gi - gx0));
                uint32_t ov[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint4 v4 = orw[q];
                    ov[4 * q] = v4.x;
                    ov[4 * q + 1] = v4.y;
                    ov[4 * q + 2] = v4.z;
                    ov[4 * q + 3] = v4.w;
                }
                blend48(w, ov);
            }
            // plain stores (nt 1.356, sc1 1.581 against 1.335 ms; round 5,
            // profiles/r05/vpass/ab_vstore_policy_r05af.txt)
            uint8_t* dp = dsb + (int64_t)rr * p.dst_pitch + 48 * gi;
#pragma unroll
            for (int q = 0; q < 3; ++q) store16<0>(dp + 16 * q, 16, true, w + 4 * q);
#pragma unroll
            for (int q = 0; q < 3; ++q) gcur[q] = gnxt[q];
        }
        return;
    }
    // General layout: 16-B chunks, byte-wise blend.  Four chunks per thread are
    // loaded before any is stored, so each wave keeps four reads in flight.
    const int chunks = (row_bytes + 15) >> 4;
    const int total = nrows * chunks;
    for (int base = threadIdx.x; base < total; base += 4 * 256) {
        uint32_t w[4][4];
        int rr[4], c0[4], nb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = base + u * 256;
            rr[u] = idx / chunks;
            c0[u] = (idx - rr[u] * chunks) << 4;
            nb[u] = idx < total ? min(16, row_bytes - c0[u]) : 0;
            if (nb[u] > 0) {
                const uint8_t* bp = bg + p.bg_off + (int64_t)(y0 + rr[u]) * p.bg_pitch + c0[u];
                load16(bp, nb[u], nb[u] == 16 && (reinterpret_cast<uintptr_t>(bp) & 15u) == 0, w[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (nb[u] <= 0) continue;
            const int o = y0 + rr[u] - p.y;
            if (any && o >= oy_lo && o < oy_hi && c0[u] + nb[u] > 3 * p.x && c0[u] < 3 * (p.x + p.ov_w)) {
                const uint32_t* orw = orow + rr[u] * os + xo;
                blend16(w[u], c0[u], nb[u], p.x, p.ov_w, [&](int ox) { return orw[ox]; });
            }
            uint8_t* dp = dst + p.dst_off + (int64_t)(y0 + rr[u]) * p.dst_pitch + c0[u];
            store16<0>(dp, nb[u], nb[u] == 16 && (reinterpret_cast<uintptr_t>(dp) & 15u) == 0, w[u]);
        }
    }
}

#if IPP_VB_WPE > 0
#define IPP_VB_ATTR __attribute__((amdgpu_waves_per_eu(IPP_VB_WPE)))
#else
#define IPP_VB_ATTR
#endif
template <bool MAGIC>
__global__ void __launch_bounds__(256) IPP_VB_ATTR
k_pipe_vblend_mfma(const uint8_t* __restrict__ tmp, const uint8_t* __restrict__ bg, uint8_t* __restrict__ dst,
                   const int32_t* __restrict__ coefs, const ipp_pipe_desc* __restrict__ descs, FastDiv tiles_y,
                   int ov_w_max, const uint16_t* __restrict__ trim, int trim_stride) {
    extern __shared__ __attribute__((aligned(16))) uint32_t orow[];  // [kBandRows][orow_stride(ov_w_max)] (+ 256 divisors)
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, tiles_y);
    const int ty = (int)(b - (uint32_t)im * tiles_y.d);
    // (trim: the H launch's trim table, trim_stride entries per item, or null)
    vblend_block<MAGIC>(orow, tmp, bg, dst, coefs, descs, im, ty, ov_w_max,
                        trim ? trim + (int64_t)im * trim_stride : nullptr);
}

// The same block over one image pointer (a scene's layers >= 1): reads the
// composite, blends the overlay, writes it back (vblend_block, INPLACE).
template <bool MAGIC>
__global__ void __launch_bounds__(256) IPP_VB_ATTR
k_pipe_vblend_over(const uint8_t* __restrict__ tmp, uint8_t* img, const int32_t* __restrict__ coefs,
                   const ipp_pipe_desc* __restrict__ descs, FastDiv tiles_y, int ov_w_max) {
    extern __shared__ __attribute__((aligned(16))) uint32_t orow[];  // as k_pipe_vblend_mfma
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const int im = (int)fdiv(b, tiles_y);
    const int ty = (int)(b - (uint32_t)im * tiles_y.d);
    // (no trim table: the later layers' T comes from ipp_pipe_hpass, written in full)
    vblend_block<MAGIC, true>(orow, tmp, img, img, coefs, descs, im, ty, ov_w_max, nullptr);
}

// bg == nullptr: the in-place form (ipp_pipe_vblend_over) on dst.  trim: the
// H launch's trim table (trim_bands(max_rows) entries per item) or null.
int vblend_entry(const uint8_t* tmp, const uint8_t* bg, uint8_t* dst, const int32_t* coefs,
                 const ipp_pipe_desc* descs, int32_t n_images, int32_t bg_w, int32_t bg_h, int32_t max_ov_w,
                 int32_t max_ov_h, int32_t tap_format, const uint16_t* trim, int32_t max_rows, void* stream) {
    if (n_images == 0) return IPP_OK;
    if (!tmp || !dst || !coefs || !descs || n_images < 0 || bg_w <= 0 || bg_h <= 0) return IPP_E_ARG;
    if (trim && (max_rows <= 0 || !bg)) return IPP_E_ARG;
    if (tap_format != IPP_TAPS_MFMA || max_ov_w <= 0 || max_ov_w > bg_w || max_ov_h <= 0 || max_ov_h > bg_h ||
        max_ov_w > IPP_PIPE_MAX_OV_W)
        return IPP_E_ARG;
    const size_t rows = (size_t)kBandRows * orow_stride(max_ov_w) * sizeof(uint32_t);
    const size_t magic = 256 * sizeof(uint32_t);  // the unpremultiply divisors, when they fit beside the rows
    const bool use_magic = rows + magic <= 64 * 1024;
    const int tyb = std::min(paste_max_bands(max_ov_h), (bg_h + kBandRows - 1) / kBandRows);
    const int64_t nb = (int64_t)tyb * n_images;
    if (nb >= INT32_MAX) return IPP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const FastDiv ftyb = fast_div((uint32_t)tyb);
    if (!bg) {
        if (use_magic)
            hipLaunchKernelGGL(k_pipe_vblend_over<true>, dim3((uint32_t)nb), dim3(256), rows + magic, st, tmp, dst,
                               coefs, descs, ftyb, max_ov_w);
        else
            hipLaunchKernelGGL(k_pipe_vblend_over<false>, dim3((uint32_t)nb), dim3(256), rows, st, tmp, dst, coefs,
                               descs, ftyb, max_ov_w);
        IPP_CHECK_LAUNCH();
        return IPP_OK;
    }
    const int tstride = trim ? trim_bands(max_rows) : 0;
    if (use_magic)
        hipLaunchKernelGGL(k_pipe_vblend_mfma<true>, dim3((uint32_t)nb), dim3(256), rows + magic, st, tmp, bg, dst,
                           coefs, descs, ftyb, max_ov_w, trim, tstride);
    else
        hipLaunchKernelGGL(k_pipe_vblend_mfma<false>, dim3((uint32_t)nb), dim3(256), rows, st, tmp, bg, dst, coefs,
                           descs, ftyb, max_ov_w, trim, tstride);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

}  // namespace

extern "C" int ipp_pipe_vblend_bands(const uint8_t* tmp, const uint8_t* bg, uint8_t* dst, const int32_t* coefs,
                                     const ipp_pipe_desc* descs, int32_t n_images, int32_t bg_w, int32_t bg_h,
                                     int32_t max_ov_w, int32_t max_ov_h, int32_t tap_format, void* stream) {
    return ipp_pipe_vblend_bands_trim(tmp, bg, dst, coefs, descs, n_images, bg_w, bg_h, max_ov_w, max_ov_h, tap_format,
                                      nullptr, 0, stream);
}

extern "C" int ipp_pipe_vblend_bands_trim(const uint8_t* tmp, const uint8_t* bg, uint8_t* dst, const int32_t* coefs,
                                          const ipp_pipe_desc* descs, int32_t n_images, int32_t bg_w, int32_t bg_h,
                                          int32_t max_ov_w, int32_t max_ov_h, int32_t tap_format,
                                          const uint16_t* trim, int32_t max_rows, void* stream) {
    if (n_images == 0) return IPP_OK;
    if (!bg) return IPP_E_ARG;
    return vblend_entry(tmp, bg, dst, coefs, descs, n_images, bg_w, bg_h, max_ov_w, max_ov_h, tap_format, trim,
                        max_rows, stream);
}

extern "C" int ipp_pipe_vblend_over(const uint8_t* tmp, uint8_t* dst, const int32_t* coefs,
                                    const ipp_pipe_desc* descs, int32_t n_images, int32_t bg_w, int32_t bg_h,
                                    int32_t max_ov_w, int32_t max_ov_h, int32_t tap_format, void* stream) {
    return vblend_entry(tmp, nullptr, dst, coefs, descs, n_images, bg_w, bg_h, max_ov_w, max_ov_h, tap_format, nullptr,
                        0, stream);
}
