// Baseline JPEG files decoded on the device to the RGB pixels libjpeg-turbo
// (Pillow's Image.open(f).convert("RGB")) gives, value for value (ipp.h:
// ipp_jpeg_decode; the rule — dequantisation, the islow inverse transform, the
// 4:2:0 upsampling with its w <= 4 case, the colour conversion — is stated
// there and in DESIGN.md §3).  All arithmetic is int32/uint32; no float.
//
// The host (jpeg.py parse_jpeg) walks the markers; the device gets each file's
// entropy-coded span, its tables and a descriptor.  Blocks are numbered in scan
// order as in ipp_jpeg.hip (4:2:0: MCU m holds 6m .. 6m + 5 = Y00 Y01 Y10 Y11
// Cb Cr; 4:4:4: 3m .. 3m + 2).  A segment is a restart interval, or the scan.
//   k_jpegd_segs  one workgroup per image: finds the RSTn markers of the span,
//                 checks their order and count, writes the segments' byte
//                 ranges and the image's status word.
//   k_jpegd_zero  zeroes the coefficient scratch (the decoder writes only the
//                 nonzero terms).
//   k_jpegd_huff  one workgroup per segment.  The segment is cut into
//                 subsequences of kSub bytes; lane i decodes subsequence i from
//                 an assumed state (start of an MCU), then rounds in which lane
//                 i + 1 restarts from lane i's end (bit, block of the MCU,
//                 coefficient index) run until no lane's start changes — the
//                 fixed point, at most as many rounds as subsequences, and it
//                 is the sequential decode because lane 0's start is the true
//                 one.
//   k_jpegd_write one workgroup per segment.  A scan of the per-lane block
//                 counts gives the write positions, and the segment is checked:
//                 whole, no more.  Then each lane once more from its now true
//                 start: writes the int16 terms, zigzag undone.
//   k_jpegd_dc    one workgroup per segment: per component the running sum of
//                 the DC differences.
//   k_jpegd_idct  one workgroup per 128 x 128 px tile: the chroma blocks of the
//                 tile (4:2:0: and one block of halo) are transformed into LDS,
//                 then one thread per luma block transforms it in registers,
//                 upsamples the chroma from LDS, converts and stores RGB.
// An image with a nonzero status is not touched by k_jpegd_idct: its output is
// left unwritten.  Every index is bounded where it is used: the bit reader by
// the segment's end, block indices by the segment's block count, coefficient
// indices by 63, table indices by the tables' sizes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ipp.h"
#include "ipp_device.h"

#ifndef IPP_JPEGD_SUBSEQ
#define IPP_JPEGD_SUBSEQ 128   // bytes of a subsequence (DESIGN.md §3 has the figures behind it)
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSub = IPP_JPEGD_SUBSEQ;
constexpr int kMaxImages = 65535;                 // gridDim.y
constexpr int kTile = 128;                        // px side of a k_jpegd_idct tile: 16 x 16 luma blocks
constexpr int kHtabBytes = 16 + 256;              // BITS, HUFFVAL of one table
constexpr uint64_t kNoStart = ~0ull;   // a lane that has not decoded yet (no key: bit positions stay below 2^34)

__constant__ const uint8_t kZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One subsequence's record in the scratch.
struct Sub {
    uint64_t start, end;   // keys: bit position in the span << 16 | block of the MCU << 8 | coefficient index
    uint32_t n, excl;      // blocks completed in the subsequence; those completed before it in the segment
};

struct Geo {
    int bpm, mcux, mcuy, nmcu, nseg, ri;   // ri: MCUs per segment
    int64_t nblk;
};

__host__ __device__ inline Geo geo_of(const ipp_jpegd_desc& d) {
    Geo g;
    const int mcu = d.sampling == IPP_JPEG_420 ? 16 : 8;
    g.bpm = d.sampling == IPP_JPEG_420 ? 6 : 3;
    g.mcux = (d.w + mcu - 1) / mcu, g.mcuy = (d.h + mcu - 1) / mcu;
    g.nmcu = g.mcux * g.mcuy;
    g.ri = d.restart > 0 && d.restart < g.nmcu ? d.restart : g.nmcu;
    g.nseg = (g.nmcu + g.ri - 1) / g.ri;
    g.nblk = (int64_t)g.nmcu * g.bpm;
    return g;
}

inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

// Bytes of the three scratch parts of one image: coefficients, subsequence
// records (a segment of len bytes at byte a of the span, the k-th, uses the
// records from a / kSub + k on: ⌈len / kSub⌉ of them, disjoint from the next
// segment's), segment ranges.
inline void parts_of(const ipp_jpegd_desc& d, int64_t (&bytes)[3]) {
    const Geo g = geo_of(d);
    bytes[0] = up256(g.nblk * 128);
    bytes[1] = up256(((int64_t)d.span_len / kSub + g.nseg + 1) * (int64_t)sizeof(Sub));
    bytes[2] = up256((int64_t)g.nseg * 8);
}

inline bool shape_ok(const ipp_jpegd_desc& d) {
    return d.w >= 1 && d.h >= 1 && d.w <= IPP_JPEG_MAX_SIDE && d.h <= IPP_JPEG_MAX_SIDE &&
           (d.sampling == IPP_JPEG_420 || d.sampling == IPP_JPEG_444) && d.restart >= 0 && d.restart <= 65535 &&
           d.span_len >= 0 && d.span_len <= IPP_JPEGD_MAX_SPAN;
}

__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* s_sum, uint32_t& all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += up;
    }
    if (lane == 63u) s_sum[wave] = inc;
    __syncthreads();
    uint32_t before = 0u;
    all = 0u;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kWaves; ++k) {
        if (k < wave) before += s_sum[k];
        all += s_sum[k];
    }
    __syncthreads();   // s_sum may be rewritten by the caller's next step
    return before + inc - v;
}

// ---- segments --------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_jpegd_segs(const uint8_t* __restrict__ data,
                                                         const ipp_jpegd_desc* __restrict__ descs,
                                                         uint8_t* __restrict__ scratch, int32_t* __restrict__ stat) {
    __shared__ uint32_t s_sum[kWaves];
    __shared__ int s_err;
    const int64_t image = blockIdx.x;
    const ipp_jpegd_desc& d = descs[image];
    const Geo g = geo_of(d);
    const uint8_t* raw = data + d.span_off;
    const int64_t len = d.span_len;
    int32_t* seg = reinterpret_cast<int32_t*>(scratch + d.seg_off);
    if (threadIdx.x == 0u) s_err = 0;
    __syncthreads();
    int err = 0;
    uint32_t carry = 0u;
    for (int64_t base = 0; base < len; base += kThreads * 16) {
        const int64_t at = base + (int64_t)threadIdx.x * 16;
        uint32_t mine = 0u;
        for (int e = 0; e < 16; ++e) {
            const int64_t x = at + e;
            if (x >= len || raw[x] != 0xFFu) continue;
            if (x + 1 >= len) {
                err = max(err, IPP_JPEGD_TRUNCATED);
                continue;
            }
            const uint32_t nx = raw[x + 1];
            if (nx == 0u) continue;
            if (nx >= 0xD0u && nx <= 0xD7u) ++mine;
            else err = max(err, IPP_JPEGD_BAD_MARKER);   // fill bytes (FF FF) included
        }
        uint32_t all;
        uint32_t k = carry + block_exclusive(mine, s_sum, all);
        for (int e = 0; e < 16 && mine > 0u; ++e) {
            const int64_t x = at + e;
            if (x + 1 >= len || raw[x] != 0xFFu) continue;
            const uint32_t nx = raw[x + 1];
            if (nx < 0xD0u || nx > 0xD7u) continue;
            if (k + 1u < (uint32_t)g.nseg) {
                if (nx - 0xD0u != (k & 7u)) err = max(err, IPP_JPEGD_WRONG_RST);
                seg[2 * k + 1] = (int32_t)x;
                seg[2 * k + 2] = (int32_t)(x + 2);
            } else {
                err = max(err, IPP_JPEGD_SEG_COUNT);
            }
            ++k;
        }
        carry += all;
    }
    if (carry + 1u != (uint32_t)g.nseg) err = max(err, IPP_JPEGD_SEG_COUNT);
    if (err) atomicMax(&s_err, err);
    __syncthreads();
    if (threadIdx.x == 0u) {
        seg[0] = 0;
        seg[2 * (g.nseg - 1) + 1] = (int32_t)len;
        int32_t* st = stat + IPP_JPEGD_STAT * image;
        st[0] = s_err, st[1] = 0, st[2] = 0, st[3] = s_err;
    }
}

__global__ __launch_bounds__(kThreads) void k_jpegd_zero(const ipp_jpegd_desc* __restrict__ descs,
                                                         uint8_t* __restrict__ scratch) {
    const ipp_jpegd_desc& d = descs[blockIdx.y];
    const int64_t at = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (at >= geo_of(d).nblk * 128) return;
    *reinterpret_cast<uint4*>(scratch + d.coef_off + at) = make_uint4(0u, 0u, 0u, 0u);
}

// ---- entropy decode --------------------------------------------------------
// A Huffman table in LDS, built from BITS / HUFFVAL (Annex C / F.2.2.3): a
// code of length l read left-aligned in 16 bits is below lim[l]; its symbol is
// vals[(off[l] + (code >> (16 - l))) & 255].  look[] answers codes of up to 8
// bits at once: length << 8 | symbol, 0 where the code is longer.
struct HTab {
    uint32_t lim[17];
    int32_t off[17];
    uint16_t look[256];
    uint8_t vals[256];
};

__device__ __forceinline__ bool huff_slow(const HTab& t, uint32_t code16, int maxlen, uint32_t& len, uint32_t& sym) {
    uint32_t l = 1u;   // lim[] does not decrease: the length is one more than the limits at or below the code
#pragma unroll
    for (int i = 1; i <= 16; ++i) l += (i <= maxlen && code16 >= t.lim[i]) ? 1u : 0u;
    if (l > (uint32_t)maxlen) return false;
    len = l;
    sym = t.vals[(uint32_t)(t.off[l] + (int32_t)(code16 >> (16u - l))) & 255u];
    return true;
}

// tabs[c] = DC table, tabs[3 + c] = AC table of component c.
__device__ void build_tabs(HTab* tabs, const uint8_t* __restrict__ htabs, const ipp_jpegd_desc& d) {
    const uint32_t tid = threadIdx.x;
    for (int t = 0; t < 6; ++t) {
        const int id = t == 0 ? d.dc[0] : t == 1 ? d.dc[1] : t == 2 ? d.dc[2] : t == 3 ? d.ac[0] : t == 4 ? d.ac[1] : d.ac[2];
        const uint8_t* src = htabs + (int64_t)id * kHtabBytes;
        tabs[t].vals[tid] = src[16 + tid];
        if (tid == 0u) {
            uint32_t code = 0u;
            int k = 0;
            tabs[t].lim[0] = 0u, tabs[t].off[0] = 0;
            for (int l = 1; l <= 16; ++l) {
                const uint32_t nb = src[l - 1];
                tabs[t].off[l] = k - (int32_t)code;
                code += nb, k += (int)nb;
                tabs[t].lim[l] = min(code << (16 - l), 65536u);
                code <<= 1;
            }
        }
    }
    __syncthreads();
    for (int t = 0; t < 6; ++t) {
        uint32_t len, sym;
        tabs[t].look[tid] = huff_slow(tabs[t], tid << 8, 8, len, sym) ? (uint16_t)((len << 8) | sym) : (uint16_t)0;
    }
    __syncthreads();
}

// 32 bits of the segment from bit position p (of the span; p is never inside a
// stuffed 0x00), stuffing skipped, 1-bits past the segment's end `endb`.  pos
// receives, 4 bits each, the span-byte offset from p >> 3 of the n-th data
// byte (n = 0..5): where a read of n bytes further on stands.
__device__ __forceinline__ uint32_t window(const uint8_t* __restrict__ raw, int endb, int64_t p, uint32_t& pos) {
    const int q = (int)(p >> 3);   // spans are at most 2^30 bytes
    // Twelve bytes: three dwords where they lie inside the segment, else byte by
    // byte up to its end and 1-bits after it.  No byte past the segment, so
    // none past the span, is read.
    uint32_t dw[3];
    const int rem = endb - q;
    if (rem >= 12) {
#pragma unroll
        for (int i = 0; i < 3; ++i) dw[i] = ld_u32_unaligned(raw + q + 4 * i);
    } else {
        dw[0] = dw[1] = dw[2] = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < 11; ++i)
            if (i < rem) dw[i >> 2] ^= (uint32_t)(raw[q + i] ^ 0xFFu) << (8 * (i & 3));
    }
    uint64_t out = 0;
    uint32_t nb = 0u, prev = 0u;
    pos = 0u;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const uint32_t b = (dw[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        // plain arithmetic, no compares: a dozen live lane masks cost more scalar registers than there are
        const uint32_t take = 1u ^ (((b - 1u) >> 31) & ((prev + 1u) >> 8));   // 0 for a stuffed byte
        prev = b;
        const uint32_t m5 = take & ((nb - 5u) >> 31), m6 = take & ((nb - 6u) >> 31);
        out = (out << (8u * m5)) | (b * m5);
        pos |= ((uint32_t)i * m6) << (4u * (nb & 7u));
        nb += take;
    }
    return (uint32_t)((out << (24u + (uint32_t)(p & 7))) >> 32);
}

__device__ __forceinline__ int extend(uint32_t v, uint32_t s) {
    return v < (1u << (s - 1u)) ? (int)v - (int)((1u << s) - 1u) : (int)v;
}

// Decodes from `key` until a symbol starts at or past bit `limit` (or the
// segment's bits run out) and returns the key there; n receives the blocks
// completed (low 24 bits) and the largest fault met (high 8).  A fault does
// not stop the lane: from a wrong start faults are the rule, and a lane that
// stopped could never fall into step with the stream.  It goes on by a fixed
// rule (a run past 63 ends the block; bits that are no code are skipped one
// at a time), and at the fixed point, where every start is true, a fault is
// the stream's own.  WRITE: stores the terms of block cur (< nblk_seg) of the
// segment's coefficients.
// The end of a segment's data: a stuffed 0x00 that closes it (the padded last
// byte came out as 0xFF) carries no bit.
__device__ __forceinline__ int data_end(const uint8_t* __restrict__ raw, int a, int b) {
    return b - a >= 2 && raw[b - 1] == 0u && raw[b - 2] == 0xFFu ? b - 1 : b;
}

template <bool WRITE>
__device__ uint64_t decode_sub(const uint8_t* __restrict__ raw, int endb, uint64_t key, int64_t limit,
                               const HTab* tabs, int bpm, bool s420, uint32_t& n, int16_t* coef, uint32_t cur,
                               uint32_t nblk_seg) {
    n = 0u;
    uint32_t err = 0u;
    int64_t p = (int64_t)(key >> 16);
    uint32_t j = (uint32_t)(key >> 8) & 0xFFu, k = (uint32_t)key & 0xFFu;
    const int64_t endbits = (int64_t)endb * 8;
    while (p < limit) {
        uint32_t pos;
        const uint32_t bits = window(raw, endb, p, pos);
        const uint32_t comp = s420 ? (j < 4u ? 0u : j - 3u) : j;
        const HTab& t = tabs[(k == 0u ? 0u : 3u) + min(comp, 2u)];
        uint32_t len, sym, fault = 0u;
        uint32_t total, at = 64u, knext = k, s = 0u;   // at: coefficient index a value goes to
        const uint32_t e = t.look[bits >> 24];
        bool found = true;
        if (e != 0u) len = e >> 8, sym = e & 0xFFu;
        else found = huff_slow(t, bits >> 16, 16, len, sym);
        if (!found) {
            if (p + 16 > endbits) break;   // fewer than 16 bits left and no code among them: the padding's 1-bits
            fault = IPP_JPEGD_BAD_CODE, total = 1u;   // goes on one bit further, in the same state
        } else if (k == 0u) {
            s = sym & 15u;
            if (sym > 11u) fault = IPP_JPEGD_BAD_CODE;
            total = len + s, at = 0u, knext = 1u;
        } else if ((sym & 15u) == 0u) {
            const uint32_t run = sym >> 4;
            total = len, knext = 64u;
            if (run == 15u) {
                if (k + 16u > 63u) fault = IPP_JPEGD_RUN;
                else knext = k + 16u;
            } else if (run != 0u) {
                fault = IPP_JPEGD_BAD_CODE;
            }
        } else {
            const uint32_t run = sym >> 4;
            s = sym & 15u;
            if (s > 10u) fault = IPP_JPEGD_BAD_CODE;
            total = len + s;
            if (k + run > 63u) fault = IPP_JPEGD_RUN, knext = 64u;
            else at = k + run, knext = at + 1u;
        }
        if (p + total > endbits) break;   // the segment's padding, or a stream cut short
        err = max(err, fault);
        if (WRITE && at < 64u && s > 0u && cur < nblk_seg)
            coef[(int64_t)cur * 64 + kZZ[at]] = (int16_t)extend((bits << len) >> (32u - s), s);
        k = knext;
        if (k == 64u) {
            k = 0u, ++n, ++cur;
            if (++j == (uint32_t)bpm) j = 0u;
        }
        const uint32_t u = (uint32_t)(p & 7) + total;   // <= 34: at most 4 data bytes on
        p = (((p >> 3) + ((pos >> (4u * (u >> 3))) & 15u)) << 3) + (u & 7u);
    }
    n |= err << 24;
    return ((uint64_t)p << 16) | (j << 8) | k;
}

__global__ __launch_bounds__(kThreads) void k_jpegd_huff(const uint8_t* __restrict__ data,
                                                         const ipp_jpegd_desc* __restrict__ descs,
                                                         const uint8_t* __restrict__ htabs, uint8_t* scratch,
                                                         int32_t* stat) {
    __shared__ HTab s_tabs[6];
    const int64_t image = blockIdx.y;
    const ipp_jpegd_desc& d = descs[image];
    const Geo g = geo_of(d);
    int32_t* st = stat + IPP_JPEGD_STAT * image;
    const int sidx = (int)blockIdx.x;
    if (sidx >= g.nseg || st[3] != 0) return;   // block-uniform; st[3] is k_jpegd_segs' alone
    build_tabs(s_tabs, htabs, d);
    const int32_t* seg = reinterpret_cast<const int32_t*>(scratch + d.seg_off);
    const uint8_t* raw = data + d.span_off;
    const int a = seg[2 * sidx], b = data_end(raw, a, seg[2 * sidx + 1]);
    const int nsub = (b - a + kSub - 1) / kSub;
    Sub* sub = reinterpret_cast<Sub*>(scratch + d.sub_off) + (a / kSub + sidx);
    const bool s420 = d.sampling == IPP_JPEG_420;
    const int tid = (int)threadIdx.x;
    auto limit_of = [&](int i) { return (int64_t)min(a + (i + 1) * kSub, b) * 8; };

    // The assumed states: lane i + 1 starts an MCU at its first byte, written
    // as lane i's end with no start yet, so that the first round decodes every
    // lane from it (lane 0's start is the true state).
    for (int i = tid; i < nsub; i += kThreads) {
        int q = a + (i + 1) * kSub;
        if (q < b && raw[q] == 0u && raw[q - 1] == 0xFFu) ++q;   // a stuffed byte is no data
        Sub r;
        r.start = kNoStart, r.end = ((uint64_t)q * 8) << 16, r.n = 0u, r.excl = 0u;
        sub[i] = r;
    }
    __syncthreads();
    // Rounds to the fixed point: lane i restarts where lane i - 1 ended, while
    // any lane's start changes.
    __shared__ int s_changed;
    if (tid == 0) s_changed = 0;
    int rounds = 0;
    for (;;) {
        int changed = 0;
        for (int base = 0; base < nsub; base += kThreads) {
            const int i = base + tid;
            uint64_t from = ((uint64_t)a * 8) << 16;
            if (i > 0 && i < nsub) from = sub[i - 1].end;
            const bool redo = i < nsub && from != sub[i].start;
            __syncthreads();
            if (redo) {
                Sub r;
                r.start = from;
                r.end = decode_sub<false>(raw, b, from, limit_of(i), s_tabs, g.bpm, s420, r.n, nullptr, 0u, 0u);
                r.excl = 0u;
                sub[i] = r;
                changed = 1;
            }
            __syncthreads();
        }
        if (changed) s_changed = 1;
        __syncthreads();
        const int any = s_changed;
        __syncthreads();
        if (!any) break;
        if (tid == 0) s_changed = 0;
        ++rounds;
    }
    if (tid == 0) {
        atomicMax(&st[1], rounds);   // the rounds in which a lane decoded; one more confirmed them
        atomicMax(&st[2], nsub);
    }
}

// Once every start state is the true one: the blocks before each subsequence,
// the check that the segment is whole (its block count, an MCU boundary, less
// than a byte left), and the last pass — the terms, zigzag undone, into the
// zeroed coefficient scratch.
__global__ __launch_bounds__(kThreads) void k_jpegd_write(const uint8_t* __restrict__ data,
                                                          const ipp_jpegd_desc* __restrict__ descs,
                                                          const uint8_t* __restrict__ htabs, uint8_t* scratch,
                                                          int32_t* stat) {
    __shared__ HTab s_tabs[6];
    __shared__ uint32_t s_sum[kWaves];
    const int64_t image = blockIdx.y;
    const ipp_jpegd_desc& d = descs[image];
    const Geo g = geo_of(d);
    const int sidx = (int)blockIdx.x;
    int32_t* st = stat + IPP_JPEGD_STAT * image;
    if (sidx >= g.nseg || st[3] != 0) return;   // block-uniform; st[3] is k_jpegd_segs' alone
    const int tid = (int)threadIdx.x;
    build_tabs(s_tabs, htabs, d);
    const int32_t* seg = reinterpret_cast<const int32_t*>(scratch + d.seg_off);
    const uint8_t* raw = data + d.span_off;
    const int a = seg[2 * sidx], b = data_end(raw, a, seg[2 * sidx + 1]);
    const int nsub = (b - a + kSub - 1) / kSub;
    const uint32_t nblk_seg = (uint32_t)(min(g.ri, g.nmcu - sidx * g.ri) * g.bpm);
    Sub* sub = reinterpret_cast<Sub*>(scratch + d.sub_off) + (a / kSub + sidx);
    int16_t* coef = reinterpret_cast<int16_t*>(scratch + d.coef_off) + (int64_t)sidx * g.ri * g.bpm * 64;
    // the blocks before each subsequence, and the largest fault of any lane
    __shared__ int s_fault;
    if (tid == 0) s_fault = 0;
    __syncthreads();
    uint32_t carry = 0u;
    for (int base = 0; base < nsub; base += kThreads) {
        const int i = base + tid;
        const uint32_t v = i < nsub ? sub[i].n : 0u;
        if (v >> 24) atomicMax(&s_fault, (int)(v >> 24));
        uint32_t all;
        const uint32_t ex = block_exclusive(v & 0xFFFFFFu, s_sum, all);
        if (i < nsub) sub[i].excl = carry + ex;
        carry += all;
    }
    __syncthreads();
    const uint64_t last = nsub > 0 ? sub[nsub - 1].end : (((uint64_t)a * 8) << 16);
    int err = s_fault;
    if (err == 0 && (carry != nblk_seg || (last & 0xFFFFu) != 0u || (int64_t)b * 8 - (int64_t)(last >> 16) >= 8))
        err = IPP_JPEGD_SEG_BLOCKS;
    if (err) {   // block-uniform: nothing of a bad segment is written
        if (tid == 0) atomicMax(&st[0], err);
        return;
    }
    for (int i = tid; i < nsub; i += kThreads) {
        uint32_t n;
        decode_sub<true>(raw, b, sub[i].start, (int64_t)min(a + (i + 1) * kSub, b) * 8, s_tabs, g.bpm,
                         d.sampling == IPP_JPEG_420, n, coef, sub[i].excl, nblk_seg);
    }
}

// ---- DC predictors ---------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_jpegd_dc(const ipp_jpegd_desc* __restrict__ descs,
                                                       uint8_t* __restrict__ scratch, const int32_t* __restrict__ stat) {
    __shared__ uint32_t s_sum[kWaves];
    const int64_t image = blockIdx.y;
    const ipp_jpegd_desc& d = descs[image];
    const Geo g = geo_of(d);
    const int sidx = (int)blockIdx.x;
    if (sidx >= g.nseg || stat[IPP_JPEGD_STAT * image] != 0) return;
    const int nm = min(g.ri, g.nmcu - sidx * g.ri);
    int16_t* coef = reinterpret_cast<int16_t*>(scratch + d.coef_off) + (int64_t)sidx * g.ri * g.bpm * 64;
    const bool s420 = d.sampling == IPP_JPEG_420;
    for (int c = 0; c < 3; ++c) {
        const int per = s420 && c == 0 ? 4 : 1, j0 = s420 ? (c == 0 ? 0 : 3 + c) : c;
        const int count = nm * per;
        uint32_t carry = 0u;
        for (int base = 0; base < count; base += kThreads) {
            const int t = base + (int)threadIdx.x;
            int16_t* at = coef + ((int64_t)(t / per) * g.bpm + j0 + t % per) * 64;
            const uint32_t v = t < count ? (uint32_t)(int)*at : 0u;
            uint32_t all;
            const uint32_t ex = block_exclusive(v, s_sum, all);
            if (t < count) *at = (int16_t)(carry + ex + v);
            carry += all;
        }
    }
}

// ---- dequantise, inverse transform, upsample, colour -----------------------
// jidctint.c, one pass over eight values: outputs (x + 2^(S-1)) >> S.
template <int S>
__device__ __forceinline__ void idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int rnd = 1 << (S - 1);
    int z1 = (d2 + d6) * 4433;
    const int t2 = z1 - d6 * 15137, t3 = z1 + d2 * 6270;
    const int t0 = (d0 + d4) << 13, t1 = (d0 - d4) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = d7, a1 = d5, a2 = d3, a3 = d1;
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
    d0 = (t10 + a3 + rnd) >> S, d7 = (t10 - a3 + rnd) >> S;
    d1 = (t11 + a2 + rnd) >> S, d6 = (t11 - a2 + rnd) >> S;
    d2 = (t12 + a1 + rnd) >> S, d5 = (t12 - a1 + rnd) >> S;
    d3 = (t13 + a0 + rnd) >> S, d4 = (t13 - a0 + rnd) >> S;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// The 64 samples (0..255) of a block from its coefficients (natural order).
__device__ __forceinline__ void block_samples(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt,
                                              int (&ws)[64]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = reinterpret_cast<const uint4*>(coef)[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t dw = (e >> 1) == 0 ? v.x : (e >> 1) == 1 ? v.y : (e >> 1) == 2 ? v.z : v.w;
            const int c = (int)(int16_t)(uint16_t)((e & 1) ? dw >> 16 : dw & 0xFFFFu);
            ws[8 * i + e] = c * (int)qt[8 * i + e];
        }
    }
#pragma unroll
    for (int x = 0; x < 8; ++x)
        idct8<11>(ws[x], ws[8 + x], ws[16 + x], ws[24 + x], ws[32 + x], ws[40 + x], ws[48 + x], ws[56 + x]);
#pragma unroll
    for (int r = 0; r < 8; ++r)
        idct8<18>(ws[8 * r], ws[8 * r + 1], ws[8 * r + 2], ws[8 * r + 3], ws[8 * r + 4], ws[8 * r + 5], ws[8 * r + 6],
                  ws[8 * r + 7]);
#pragma unroll
    for (int i = 0; i < 64; ++i) ws[i] = clamp255(ws[i] + 128);
}

constexpr int kChromaLds = 2 * kTile * kTile;   // 4:4:4: two 128 x 128 planes; 4:2:0 uses 2 x 80 x 80 of it

__global__ __launch_bounds__(kThreads) void k_jpegd_idct(const ipp_jpegd_desc* __restrict__ descs,
                                                         const uint16_t* __restrict__ qtabs,
                                                         const uint8_t* __restrict__ scratch,
                                                         const int32_t* __restrict__ stat, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_c[kChromaLds];
    const int64_t image = blockIdx.y;
    const ipp_jpegd_desc& d = descs[image];
    const int tiles_x = (d.w + kTile - 1) / kTile, tiles_y = (d.h + kTile - 1) / kTile;
    if ((int)blockIdx.x >= tiles_x * tiles_y || stat[IPP_JPEGD_STAT * image] != 0) return;   // block-uniform
    const Geo g = geo_of(d);
    const bool s420 = d.sampling == IPP_JPEG_420;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int16_t* coef = reinterpret_cast<const int16_t*>(scratch + d.coef_off);
    // chroma blocks of the tile: 4:2:0 8 x 8 and a ring of one, 4:4:4 16 x 16
    const int side = s420 ? 10 : 16, lw = side * 8;
    const int cb0x = s420 ? tx * 8 - 1 : tx * 16, cb0y = s420 ? ty * 8 - 1 : ty * 16;   // also MCU coordinates
    int ws[64];
    for (int idx = (int)threadIdx.x; idx < 2 * side * side; idx += kThreads) {
        const int c = idx / (side * side), rem = idx - c * side * side;
        const int lby = rem / side, lbx = rem - lby * side;
        const int gx = cb0x + lbx, gy = cb0y + lby;
        if (gx < 0 || gy < 0 || gx >= g.mcux || gy >= g.mcuy) continue;
        const int64_t b = ((int64_t)gy * g.mcux + gx) * g.bpm + (s420 ? 4 : 1) + c;
        block_samples(coef + b * 64, qtabs + (int64_t)(c == 0 ? d.qt[1] : d.qt[2]) * 64, ws);
        uint8_t* dst = s_c + (c * side * 8 + lby * 8) * lw + lbx * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint32_t lo = 0u, hi = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) lo |= (uint32_t)ws[8 * r + e] << (8 * e), hi |= (uint32_t)ws[8 * r + 4 + e] << (8 * e);
            *reinterpret_cast<uint2*>(dst + r * lw) = make_uint2(lo, hi);
        }
    }
    __syncthreads();
    const int bx = tx * 16 + ((int)threadIdx.x & 15), by = ty * 16 + ((int)threadIdx.x >> 4);
    if (bx * 8 >= d.w || by * 8 >= d.h) return;
    const int64_t b = s420 ? ((int64_t)(by >> 1) * g.mcux + (bx >> 1)) * 6 + (by & 1) * 2 + (bx & 1)
                           : ((int64_t)by * g.mcux + bx) * 3;
    block_samples(coef + b * 64, qtabs + (int64_t)d.qt[0] * 64, ws);
    const int cw = (d.w + 1) >> 1, ch = (d.h + 1) >> 1;
    const int ox = cb0x * 8, oy = cb0y * 8;   // chroma sample at the LDS planes' origin
    const int plane = side * 8 * lw;
    const bool fancy = cw > 2;
    // the eight chroma values of plane c under pixel row py of this block
    auto chroma_row = [&](int c, int py, int (&o)[8]) {
        const uint8_t* pl = s_c + c * plane;
        if (!s420) {
#pragma unroll
            for (int x = 0; x < 8; ++x) o[x] = pl[(py - oy) * lw + bx * 8 + x - ox];
            return;
        }
        const int cy = py >> 1;
        const int fy = min(max((py & 1) ? cy + 1 : cy - 1, 0), ch - 1);
        const uint8_t* near = pl + (cy - oy) * lw - ox;
        const uint8_t* far = pl + (fy - oy) * lw - ox;
        if (fancy) {
            int s0 = 0, s1 = 0, s2 = 0;   // chroma columns 4bx - 1 .. 4bx + 4, clamped to the plane
#pragma unroll
            for (int x = 0; x < 6; ++x) {
                const int cx = min(max(bx * 4 - 1 + x, 0), cw - 1);
                s0 = s1, s1 = s2, s2 = 3 * (int)near[cx] + (int)far[cx];
                if (x >= 2) {
                    o[2 * (x - 2)] = (3 * s1 + s0 + 8) >> 4;
                    o[2 * (x - 2) + 1] = (3 * s1 + s2 + 7) >> 4;
                }
            }
        } else {
#pragma unroll
            for (int x = 0; x < 8; ++x) o[x] = near[min(bx * 4 + (x >> 1), cw - 1)];
        }
    };
#pragma unroll
    for (int r = 0; r < 8; ++r) {   // unrolled: ws stays in registers
        const int py = by * 8 + r;
        if (py >= d.h) continue;
        int cbv[8], crv[8];
        chroma_row(0, py, cbv);
        chroma_row(1, py, crv);
        uint32_t px[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int y = ws[8 * r + x], cbm = cbv[x] - 128, crm = crv[x] - 128;
            const uint32_t rgb[3] = {(uint32_t)clamp255(y + ((91881 * crm + 32768) >> 16)),
                                     (uint32_t)clamp255(y + ((-22554 * cbm - 46802 * crm + 32768) >> 16)),
                                     (uint32_t)clamp255(y + ((116130 * cbm + 32768) >> 16))};
#pragma unroll
            for (int e = 0; e < 3; ++e) px[(3 * x + e) >> 2] |= rgb[e] << (8 * ((3 * x + e) & 3));
        }
        uint8_t* dst = out + d.out_off + (int64_t)py * d.out_pitch + (int64_t)bx * 24;
        if (bx * 8 + 8 <= d.w && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) reinterpret_cast<uint32_t*>(dst)[i] = px[i];
        } else {
            const int nbytes = min(8, d.w - bx * 8) * 3;
#pragma unroll
            for (int i = 0; i < 24; ++i)
                if (i < nbytes) dst[i] = (uint8_t)(px[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace

extern "C" int64_t ipp_jpeg_decode_scratch_bytes(ipp_jpegd_desc* descs, int32_t n_images) {
    if (n_images < 0 || n_images > kMaxImages || (n_images > 0 && !descs)) return IPP_E_ARG;
    int64_t at = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!shape_ok(descs[i])) return IPP_E_ARG;
        int64_t bytes[3];
        parts_of(descs[i], bytes);
        descs[i].coef_off = at, at += bytes[0];
        descs[i].sub_off = at, at += bytes[1];
        descs[i].seg_off = at, at += bytes[2];
    }
    return at;
}

extern "C" int ipp_jpeg_decode(const uint8_t* data, int64_t data_bytes, const ipp_jpegd_desc* descs_host,
                               const ipp_jpegd_desc* descs, int32_t n_images, const uint16_t* qtabs, int32_t n_qtabs,
                               const uint8_t* htabs, int32_t n_htabs, uint8_t* scratch, int64_t scratch_bytes,
                               uint8_t* out, int64_t out_bytes, int32_t* stat, void* stream) {
    if (!data || !descs_host || !descs || !qtabs || !htabs || !scratch || !out || !stat) return IPP_E_ARG;
    if (n_images < 0 || n_images > kMaxImages || n_qtabs < 1 || n_htabs < 1 || data_bytes < 0 || scratch_bytes < 0 ||
        out_bytes < 0)
        return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15u) != 0 || (reinterpret_cast<uintptr_t>(descs) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(stat) & 3u) != 0 || (reinterpret_cast<uintptr_t>(qtabs) & 1u) != 0)
        return IPP_E_ARG;
    int64_t at = 0, max_coef = 0;
    int max_seg = 0, max_tiles = 0;
    for (int i = 0; i < n_images; ++i) {
        const ipp_jpegd_desc& d = descs_host[i];
        if (!shape_ok(d)) return IPP_E_ARG;
        if (d.span_off < 0 || d.span_off > data_bytes - d.span_len) return IPP_E_ARG;
        for (int c = 0; c < 3; ++c)
            if (d.qt[c] < 0 || d.qt[c] >= n_qtabs || d.dc[c] < 0 || d.dc[c] >= n_htabs || d.ac[c] < 0 ||
                d.ac[c] >= n_htabs)
                return IPP_E_ARG;
        if (d.out_pitch < 3 * d.w || d.out_off < 0 ||
            d.out_off > out_bytes - ((int64_t)(d.h - 1) * d.out_pitch + 3 * (int64_t)d.w))
            return IPP_E_ARG;
        int64_t bytes[3];
        parts_of(d, bytes);
        if (d.coef_off != at || d.sub_off != at + bytes[0] || d.seg_off != at + bytes[0] + bytes[1]) return IPP_E_ARG;
        at += bytes[0] + bytes[1] + bytes[2];
        const Geo g = geo_of(d);
        max_coef = g.nblk * 128 > max_coef ? g.nblk * 128 : max_coef;
        max_seg = g.nseg > max_seg ? g.nseg : max_seg;
        const int tiles = ((d.w + kTile - 1) / kTile) * ((d.h + kTile - 1) / kTile);
        max_tiles = tiles > max_tiles ? tiles : max_tiles;
    }
    if (at > scratch_bytes) return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)n_images;
    hipLaunchKernelGGL(k_jpegd_segs, dim3(n), dim3(kThreads), 0, s, data, descs, scratch, stat);
    hipLaunchKernelGGL(k_jpegd_zero, dim3((uint32_t)((max_coef + kThreads * 16 - 1) / (kThreads * 16)), n),
                       dim3(kThreads), 0, s, descs, scratch);
    hipLaunchKernelGGL(k_jpegd_huff, dim3((uint32_t)max_seg, n), dim3(kThreads), 0, s, data, descs, htabs, scratch, stat);
    hipLaunchKernelGGL(k_jpegd_write, dim3((uint32_t)max_seg, n), dim3(kThreads), 0, s, data, descs, htabs, scratch,
                       stat);
    hipLaunchKernelGGL(k_jpegd_dc, dim3((uint32_t)max_seg, n), dim3(kThreads), 0, s, descs, scratch, stat);
    hipLaunchKernelGGL(k_jpegd_idct, dim3((uint32_t)max_tiles, n), dim3(kThreads), 0, s, descs, qtabs, scratch, stat,
                       out);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}
