// ipp_pipe_layout.h — the one statement of the fused pipe's shared layouts:
// the MFMA tap tiles of an axis, the H pass's scratch T, and the 16-row bands
// and 16-pixel column groups of a composite.  Its writers (ipp_host.cpp,
// ipp_taps.hip), its readers (ipp_pipe.hip, ipp_pipe_vblend.hip,
// ipp_label.hip) and the planner that sizes the buffers (ipp_plan.cpp) take
// every number of the format from here. Plain C++ for the host files, __host__ __device__ under hipcc.
//
// A change of a number (a count, a size, an offset) is made in this file
// alone.  A change of a formula's shape is made in the functions below and,
// besides, at the sites that write the same expression out with these named
// constants, because a helper function there changed the kernel's
// instruction stream:
//   ipp_pipe.hip  hpass2_body: ntiles, the bias and block pointers, the tap
//                 block indices of the first and later K steps, the T store;
//                 hpass_block's fill trim: ntiles, the T store;
//   ipp_taps.hip  k_plan_taps and stage_byte: the bias and block pointers,
//                 boff, the staged block indices, the plane stride;
//   ipp_label.hip overlay_alpha_band: the walk of the T address (alpha dword).
//
// ---------------------------------------------------------------------------
// MFMA tile format (v_mfma_i32_16x16x64_i8).  Outputs are grouped in tiles of
// 16, tile t covering outputs [16t - phase, 16t - phase + 16) ∩ [0, out)
// (phase lets the V pass align tiles with 16-row background bands: phase =
// y mod 16, so that each band needs exactly one tile); input indices are
// shifted by `shift` (the V pass's ybox_first).  For tile t:
//   hdr[t]  = (K0, nK, boff, compact)
//                                 K0 = first input column of the tile rounded
//                                 down to 16, nK = 64-column K steps, boff =
//                                 uint4 index of the tile's blocks
//   bias[16t + c] = 2^21 + 128·Σk of the tile's output c (0 for padding)
//   block (s, p), s < nK, p < 3: 64 lanes × 16 B; lane l holds bytes
//           j = 0..15 = balanced byte p of the tap of the tile's output l&15
//           at input K0 + 64s + 16(l>>4) + j (0 outside its support).  This is
//           the B operand B[k][col] of the H pass and, unchanged, the A
//           operand A[row][k] of the V pass (same lane map).
// (each 22-bit tap k = b0 + 256 b1 + 65536 b2, b in [-128, 127]) so that with
// pixels stored XOR 0x80 the i8 MFMA accumulators give
//   2^21 + Σ p·k = bias + Σ_p 2^(8p) acc_p   exactly.
// Layout per axis (int32 units from coef_off): hdr[4T], bias[16T], blocks (4
// int32 each); dense block (s, p) of a tile is block boff + (3s + p)·64 + lane.
// Both writers, the device planner and the host's ipp_plan_mfma_tile, give
// every tile nkb K-step slots: boff = t·nkb·192.
//
// Compact tile (hdr.w = 1; axis->compact, nK >= 2 and at most 64 nonzero
// 16-column groups over the tile's 16 outputs): the tile's first 4 blocks
// (bytes 0..63) hold meta[16], meta[n] = g0 | len << 8 | base << 16 (output
// n's taps lie in the 16-column groups g0 .. g0 + len - 1 counted from K0;
// base = the sum of len over the outputs before n); plane p's group block i
// (16 signed bytes) is block 4 + 64 p + i, block base + j holding output n's
// group g0 + j; everything else of the tile's nkb slots is zero.  The H pass
// loads one block per lane and plane and builds each K step's B operand by
// ds_bpermute (ipp_pipe.hip), 3 loads per tile instead of 3·nK.
//
// T (the H pass's output, the V pass's input), per item: [row group g][column
// x'][4 channels][4 rows] bytes, values XOR 0x80 — one 16-B group per (g, x')
// at base + g·pitch + 16·x', channel c = dword c (alpha = dword 3).  An H-pass
// MFMA lane writes exactly one group; a V-pass lane reads four (16 T rows of
// all four channels); a K step = 64 T rows = 16 row groups.
// T is sparse after ipp_pipe_hpass_bgcopy_trim with a trim table: the groups
// the table marks constant (trim_const below; every byte of them is 0x80) are
// not stored, and the readers that take the table do not load them.
//
// Bands: composite rows outside the overlay's 16-row bands [vb0, vb1) are
// plain copies of the background (Paste.c leaves them untouched).  The H
// launch's copy blocks write them (and, column split, the band rows'
// 16-pixel groups outside the overlay's [gx0, gx1)), so the V launch only
// visits the overlay.
// ---------------------------------------------------------------------------
#pragma once
#include <stdint.h>

#include "ipp.h"

// (always inlined in the kernels: a helper inlined by the optimiser's own
// choice changes its pass order, and with it the instruction stream)
#ifdef __HIPCC__
#define IPP_HD __host__ __device__ __forceinline__
#else
#define IPP_HD inline
#endif

namespace pipe_layout {

constexpr int kTileOut = 16;       // outputs per tap tile
constexpr int kTileOutLog2 = 4;
constexpr int kKStepCols = 64;     // input columns per K step
constexpr int kTapPlanes = 3;      // balanced byte planes of a tap
constexpr int kHdrWords = 4;       // int32 of hdr per tile
constexpr int kBiasWords = kTileOut;  // int32 of bias per tile: one per output
constexpr int kKStepBlocks = kTapPlanes * kKStepCols;  // uint4 blocks per K step
constexpr int kKStepBytes = 16 * kKStepBlocks;
constexpr int kCompactMeta = 4;    // uint4 of meta before a compact tile's blocks
constexpr int kCompactBlocks = kCompactMeta + kKStepBlocks;  // uint4 a compact tile fills
constexpr int kBandRows = 16;      // composite rows of a band = rows of a V tap tile
constexpr int kTGroupRows = 4;     // T rows per group
constexpr int kTGroupRowsLog2 = 2;
constexpr int kTGroupBytes = 16;   // 4 channels × 4 rows
constexpr int kTAlphaByte = 12;    // alpha's dword in a T group
constexpr int kKStepGroups = kKStepCols / kTGroupRows;  // T row groups per K step of the V pass

IPP_HD constexpr int imin(int a, int b) { return a < b ? a : b; }
IPP_HD constexpr int imax(int a, int b) { return a > b ? a : b; }

// ---- tap axis block ---------------------------------------------------------
IPP_HD constexpr int tap_ntiles(int out_len, int phase) { return (out_len + phase + kTileOut - 1) >> kTileOutLog2; }
IPP_HD constexpr int64_t tap_bias_word(int ntiles) { return kHdrWords * (int64_t)ntiles; }
IPP_HD constexpr int64_t tap_block_word(int ntiles) { return (kHdrWords + kBiasWords) * (int64_t)ntiles; }
IPP_HD constexpr int tap_dense_block(int ks, int plane, int lane) { return (ks * kTapPlanes + plane) * kKStepCols + lane; }
IPP_HD constexpr int tap_compact_block(int plane, int i) { return kCompactMeta + plane * kKStepCols + i; }
IPP_HD constexpr int64_t tap_tile_block(int t, int nkb) { return (int64_t)t * nkb * kKStepBlocks; }
// int32 an axis of ntiles tiles with nkb K-step slots each takes
IPP_HD constexpr int64_t tap_axis_words(int64_t ntiles, int nkb) {
    return (kHdrWords + kBiasWords) * ntiles + ntiles * nkb * (kKStepBytes / 4);
}

// ---- V tiles and bands ------------------------------------------------------
IPP_HD constexpr int tap_phase(int y) { return y & (kBandRows - 1); }
// the tap tile of the band whose first composite row is y0 (overlay at row y)
IPP_HD constexpr int band_tap_tile(int y0, int y, int phase) { return (y0 - y + phase) >> 4; }
// the overlay's bands [vb0, vb1): composite rows, multiples of 16 but for bg_h
IPP_HD void paste_bands(const ipp_paste_desc& p, int& vb0, int& vb1) {
    vb0 = (p.y >> 4) << 4;
    vb1 = imin(p.bg_h, ((p.y + p.ov_h + 15) >> 4) << 4);
    vb1 = imax(vb1, vb0);
}
// an overlay of height H at any y spans at most ceil((15 + H) / 16) bands
IPP_HD constexpr int paste_max_bands(int max_ov_h) { return (max_ov_h + 15 + kBandRows - 1) / kBandRows; }

// ---- column split -------------------------------------------------------------
// Column split of the band rows: the overlay touches their 16-pixel groups
// [gx0, gx1).  It holds on dense rows of whole groups with a nonempty group
// range, bg_h·lr² < 2^32 for lr = the vectors per band row (the H copy's
// umulhi division stays exact) and both images 16-B aligned (aligned(), asked
// last: the kernels test their pointers, the planner lays its images out so).
template <typename Aligned>
IPP_HD bool band_cols_split(const ipp_paste_desc& p, int& gx0, int& gx1, Aligned aligned) {
    const int rb = 3 * p.bg_w;
    gx0 = imax(p.x, 0) >> 4;
    gx1 = imin((p.x + p.ov_w + 15) >> 4, p.bg_w >> 4);
    const int64_t lr = 3 * (p.bg_w >> 4);  // ≥ the split's vectors per band row
    return (p.bg_w & 15) == 0 && p.bg_pitch == rb && p.dst_pitch == rb && gx0 < gx1 &&
           (int64_t)p.bg_h * lr * lr < (1ll << 32) && aligned();
}

// ---- T ------------------------------------------------------------------------
IPP_HD constexpr int t_row_group(int row) { return row >> kTGroupRowsLog2; }
IPP_HD constexpr int t_pitch_vecs(int pitch_bytes) { return pitch_bytes >> 4; }  // 16-B groups per group row
// T row groups of an item: its rows rounded up to 16, and V tiles read up to
// 64·nK rows past their 16-aligned start
IPP_HD constexpr int64_t t_groups(int rows, int nkb_v) {
    return (((int64_t)(rows + 15) / 16) * 16 + kKStepCols * nkb_v + 16) / kTGroupRows;
}

// ---- trim table -----------------------------------------------------------------
// The H launch's record of its fill trim (ipp_pipe.hip hpass_block), one
// 16-bit entry per (item, H band): trim[item·trim_bands(max_rows) + band] =
// lo | hi << 8, the band's swept column tiles [lo, hi).  The T groups of the
// band's other column tiles hold 0x80 in every byte and, with a table, are
// neither stored nor loaded.  A block that does not trim writes (0, its tile
// count); a tile count of 255 or more is stored as 255 = no upper bound (only
// items of at most 64 tiles trim).  Bands at or past the item's lines have no
// entry: their T rows lie past every tap's support and are constant to a
// reader.  The table is the one source of the bounds: they come out of
// float32 arithmetic in hpass_block, which no reader repeats.
//
// H band hb = T rows 16·hb .. 16·hb + 15 of the item.  A V tile's window
// starts at T row K0, a multiple of 16 (above: K0 is rounded down to 16), and
// the V axis's input index 0 is T row 0: the planner gives the axis shift =
// the H desc's line0 (ipp_plan.cpp; both 0 when an axis is the identity), and
// T row r is M row line0 + r.  So the four groups a V lane reads in K step ks
// (rows K0 + 64·ks + 16·(lane >> 4) .. + 15) are exactly H band
// trim_v_band(K0, ks, lane).
constexpr int kTrimOpen = 255;                       // hi: no upper bound
constexpr uint32_t kTrimNone = kTrimOpen << 8;       // no group is constant (no table given)
constexpr uint32_t kTrimAll = 0;                     // every group is constant (a band past the item's lines)
IPP_HD constexpr int trim_bands(int max_rows) { return (max_rows + kBandRows - 1) / kBandRows; }
IPP_HD constexpr uint32_t trim_entry(int lo, int hi) { return (uint32_t)lo | (uint32_t)imin(hi, kTrimOpen) << 8; }
// are the T groups of column tile ct constant in the band of entry e?
IPP_HD constexpr bool trim_const(uint32_t e, int ct) {
    return ct < (int)(e & 255u) || (ct >= (int)(e >> 8 & 255u) && (e >> 8 & 255u) != (uint32_t)kTrimOpen);
}
IPP_HD constexpr int trim_v_band(int k0, int ks, int lane) { return (k0 >> 4) + (kKStepCols / kBandRows) * ks + (lane >> 4); }
static_assert(kKStepCols == 4 * kBandRows && kBandRows == 4 * kTGroupRows,
              "a V lane's four groups of a K step are one H band, a K step is four");
static_assert(trim_const(trim_entry(2, 5), 1) && !trim_const(trim_entry(2, 5), 2) && !trim_const(trim_entry(2, 5), 4) &&
                  trim_const(trim_entry(2, 5), 5) && trim_const(kTrimAll, 0) && !trim_const(kTrimNone, 300) &&
                  !trim_const(trim_entry(0, 300), 299),
              "trim_const");

static_assert(tap_block_word(1) == 20 && tap_bias_word(1) == 4, "blocks begin at word 20·T, bias at 4·T (ipp.h)");
static_assert((1 << kTileOutLog2) == kTileOut && (1 << kTGroupRowsLog2) == kTGroupRows, "the shifts");
static_assert(kKStepBytes == 3072, "3072 bytes per K step (ipp.h, ipp_plan_mfma_tile)");
static_assert(tap_tile_block(1, 1) == 192 && tap_tile_block(5, 3) == 5 * 3 * 192, "tile t's blocks at t·nkb·192 (ipp.h)");
static_assert(tap_compact_block(1, 5) == kCompactMeta + tap_dense_block(0, 1, 5), "compact blocks: the meta, then K step 0's lane map");
static_assert(tap_axis_words(1, 1) == 20 + 768 && tap_ntiles(16, 0) == 1 && tap_ntiles(16, 1) == 2, "axis size");
static_assert(kKStepGroups == 16 && kTAlphaByte == 3 * 4 && kTGroupBytes == 4 * kTGroupRows, "T group");
static_assert(paste_max_bands(1) == 1 && paste_max_bands(2) == 2 && paste_max_bands(17) == 2 && paste_max_bands(18) == 3,
              "bands of an overlay");
// the V launch keeps a band's rows of ≤ ov_w + 32 dwords in 64 KB of LDS
static_assert(kBandRows * 4 * (IPP_PIPE_MAX_OV_W + 32) == 64 * 1024, "IPP_PIPE_MAX_OV_W is the band's LDS limit");

#ifdef __HIPCC__
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// An axis's tap tiles as the kernels read them: hdr per tile (K0, nK, boff,
// compact), bias per output, and the blocks (tile t's begin at block hdr[t].z).
struct TapTiles {
    const int4* hdr;
    const int32_t* bias;
    const uint4* blk;
};
__device__ __forceinline__ TapTiles tap_tiles(const int32_t* coefs, int64_t coef_off, int ntiles) {
    return TapTiles{reinterpret_cast<const int4*>(coefs + coef_off), coefs + coef_off + tap_bias_word(ntiles),
                    reinterpret_cast<const uint4*>(coefs + coef_off + tap_block_word(ntiles))};
}

// One T group.  Group (group, x) of an item is TGroup number group·pitch + x
// from its T base, pitch = t_pitch_vecs(pitch in bytes).
typedef uint4 TGroup;
static_assert(sizeof(TGroup) == kTGroupBytes, "one 16-B vector per T group");
template <typename V>
__device__ __forceinline__ const V* t_group(const V* base, int pitch, int group, int x) {
    static_assert(sizeof(V) == kTGroupBytes, "a pointer to whole groups");
    return base + x + (int64_t)group * pitch;
}

// Column split of the band rows [vb0, vb1): on dense, 16-B aligned images
// whose width is a multiple of 16, the H pass's copy blocks also write the
// band rows' 16-pixel groups outside [gx0, gx1) (the groups the overlay
// touches) and the V pass visits only [gx0, gx1).  Both kernels decide it
// with this one predicate: the one above (ipp_plan.cpp counts the bytes by
// it) with the two images' alignment.
__device__ __forceinline__ bool band_cols_split(const ipp_paste_desc& p, const uint8_t* bg, const uint8_t* dst,
                                                int& gx0, int& gx1) {
    return pipe_layout::band_cols_split(p, gx0, gx1, [&] {
        return ((reinterpret_cast<uintptr_t>(bg + p.bg_off) | reinterpret_cast<uintptr_t>(dst + p.dst_off)) & 15u) == 0;
    });
}
#endif

}  // namespace pipe_layout
