// Baseline JPEG entropy data of RGB composites on the device, byte for byte
// what libjpeg-turbo (Pillow's Image.save) writes (ipp.h: ipp_jpeg_encode,
// ipp_jpeg_pack; the rule — colour conversion, sampling, the two edge rules,
// the islow DCT, quantisation, Huffman coding, stuffing — is stated there and
// in DESIGN.md §3).  All arithmetic is int32/uint32; there is no float.
//
// The blocks of an image are numbered in scan order (4:2:0: MCU m holds
// blocks 6m .. 6m + 5 = Y00 Y01 Y10 Y11 Cb Cr; 4:4:4: 3m .. 3m + 2 = Y Cb Cr).
//   k_jpeg_dct     one thread per block, its 64 samples in registers: colour
//                  conversion (and the 2x2 downsample) with the edge rule, the
//                  row and column passes, quantisation by a reciprocal that is
//                  exact for every operand, zigzag; writes the int16
//                  coefficients and the bit length of the AC codes.  A dummy
//                  block transforms the block whose DC it repeats and drops
//                  the AC terms.
//   k_jpeg_scan    one workgroup per image: adds each block's DC code length
//                  (against the previous block of its component) and takes
//                  the exclusive sum, 1024 blocks at a time with a carried
//                  prefix: every block's bit offset and the image's total.
//   k_jpeg_zero    zeroes the words of the unstuffed stream the total needs.
//   k_jpeg_write   one thread per block: codes its coefficients again and ORs
//                  the bits in at its offset.  The first and the last word it
//                  touches may be shared with a neighbour and are merged by
//                  atomicOr (integer, commutative: no order matters); the
//                  words between are its own and are plain stores.
//   k_jpeg_ffcount the 0xFF bytes of each 4096-B chunk of the unstuffed
//                  stream (the 1-padded last byte included).
//   k_jpeg_ffscan  one workgroup per image: the exclusive sum over its chunks;
//                  the header (stuffed byte count, status).
//   k_jpeg_stuff   scatters the bytes, a 0x00 after each 0xFF, into the slot.
//   k_jpeg_pack    (ipp_jpeg_pack) copies the slots to caller-given offsets.
// An image whose stream does not fit `capacity` is known before k_jpeg_write
// (unstuffed size) or before k_jpeg_stuff (stuffed size): nothing of it is
// written to its slot.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ipp.h"
#include "ipp_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kScanPerThread = 4;                        // blocks a thread of k_jpeg_scan sums per step
constexpr int kScanStep = kThreads * kScanPerThread;
constexpr int kChunk = kThreads * 16;                    // bytes of the unstuffed stream per workgroup (16 per thread)
constexpr int kMaxImages = 65535;                        // gridDim.y / .z

// (code << 8) | length of every symbol of the four Annex K.3 tables.
struct Huff {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

constexpr void huff_fill(uint32_t* out, const uint8_t* bits, const uint8_t* vals) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = (code++ << 8) | (uint32_t)len;
        code <<= 1;
    }
}

constexpr Huff make_huff() {
    constexpr uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    constexpr uint8_t dc_l[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    constexpr uint8_t dc_c[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
    constexpr uint8_t ac_l[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
    constexpr uint8_t ac_c[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
    constexpr uint8_t ac_l_vals[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
        0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72,
        0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
        0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
        0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
        0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
        0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
        0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
        0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
    constexpr uint8_t ac_c_vals[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
        0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1,
        0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
        0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
        0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
        0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
        0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
        0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
        0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
    Huff h{};
    huff_fill(h.dc[0], dc_l, dc_vals);
    huff_fill(h.dc[1], dc_c, dc_vals);
    huff_fill(h.ac[0], ac_l, ac_l_vals);
    huff_fill(h.ac[1], ac_c, ac_c_vals);
    return h;
}

__constant__ const Huff kHuff = make_huff();

// Natural (row-major) index of zigzag position k.
__device__ __forceinline__ constexpr int zz_nat(int k) {
    constexpr int8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k];
}

// Per table (0 luma, 1 chroma) and natural position: (m << 8) | q with the
// divisor d = 8·q and its reciprocal m = floor(2^26 / d) + 1 < 2^24.
// umulhi(a << 6, m) = (a·m) >> 26 is floor(a / d) for every a with a·d < 2^26,
// so for every a < 2^15 (d <= 2040); a = |coef| + d / 2, and |coef| <= 8·1024
// plus the passes' rounding (8 x an orthonormal DCT of samples in -128..127).
struct QTab {
    uint32_t mq[2][64];
};

// The image's geometry, everything a kernel needs (sampling 0 = 4:2:0).
struct Geo {
    int w, h, sampling, bpm;   // blocks per MCU: 6 or 3
    int mcux, mcuy, nmcu, nblk;
    int wb, hb;                // luma blocks: ⌈w / 8⌉, ⌈h / 8⌉
    FastDiv dmcux;
};

// The scratch (ipp.h): per image nblk x 64 int16 coefficients, nblk uint64
// (AC bit lengths, after the scan bit offsets), a 16-B record, the unstuffed
// stream and the per-chunk 0xFF counts.
struct Rec {
    uint64_t bits;       // total bits of the scan
    uint32_t status;
    uint32_t pad_;
};

struct Scratch {
    int16_t* coef;
    uint64_t* off;
    Rec* rec;
    uint32_t* raw;
    uint32_t* ff;
    int64_t raw_pitch;   // bytes, a multiple of 16
    int nchunk;          // ⌈raw_pitch / kChunk⌉
    int64_t total;
};

inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }
inline int64_t pitch16(int64_t v) { return (v + 15) / 16 * 16; }

inline Geo geo_of(int w, int h, int sampling) {
    Geo g;
    g.w = w, g.h = h, g.sampling = sampling;
    const int mcu = sampling == IPP_JPEG_420 ? 16 : 8;
    g.bpm = sampling == IPP_JPEG_420 ? 6 : 3;
    g.mcux = (w + mcu - 1) / mcu, g.mcuy = (h + mcu - 1) / mcu;
    g.nmcu = g.mcux * g.mcuy, g.nblk = g.nmcu * g.bpm;
    g.wb = (w + 7) / 8, g.hb = (h + 7) / 8;
    g.dmcux = fast_div((uint32_t)g.mcux);
    return g;
}

inline Scratch scratch_of(uint8_t* base, int64_t n, const Geo& g, int64_t capacity) {
    Scratch s;
    s.raw_pitch = pitch16(capacity) + 16;
    s.nchunk = (int)((s.raw_pitch + kChunk - 1) / kChunk);
    int64_t at = 0;
    s.coef = reinterpret_cast<int16_t*>(base + at), at += up256(n * g.nblk * 128);
    s.off = reinterpret_cast<uint64_t*>(base + at), at += up256(n * g.nblk * 8);
    s.rec = reinterpret_cast<Rec*>(base + at), at += up256(n * 16);
    s.raw = reinterpret_cast<uint32_t*>(base + at), at += up256(n * s.raw_pitch);
    s.ff = reinterpret_cast<uint32_t*>(base + at), at += up256(n * (int64_t)s.nchunk * 4);
    s.total = at;
    return s;
}

// jccolor.c rgb_ycc_convert for one component (wave-uniform c).
struct Ycc {
    int kr, kg, kb, add;
};
__device__ __forceinline__ Ycc ycc_of(int c) {
    if (c == 0) return Ycc{19595, 38470, 7471, 32768};
    if (c == 1) return Ycc{-11059, -21709, 32768, 128 * 65536 + 32767};
    return Ycc{32768, -27439, -5329, 128 * 65536 + 32767};
}
__device__ __forceinline__ int ycc(const Ycc& k, uint32_t r, uint32_t g, uint32_t b) {
    return (k.kr * (int)r + k.kg * (int)g + k.kb * (int)b + k.add) >> 16;
}

// Byte i (constant after unrolling) of a run of packed dwords.
template <int N>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&d)[N], int i) {
    return (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
}

// The 8x8 samples - 128 of full-resolution block (bx, by) of component k:
// columns and rows past the image repeat its last (expand_right_edge,
// expand_bottom_edge).
__device__ __forceinline__ void load_full(const uint8_t* __restrict__ img, int w, int h, int bx, int by, const Ycc& k,
                                          int (&ws)[64]) {
    const int x0 = bx * 8;
    const bool fast = x0 + 8 <= w;   // wave-divergent only in the image's last block column
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint8_t* row = img + (int64_t)min(by * 8 + r, h - 1) * w * 3;
        if (fast) {
            uint32_t d[6];   // 24 B inside the row
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i] = ld_u32_unaligned(row + (int64_t)x0 * 3 + 4 * i);
#pragma unroll
            for (int c = 0; c < 8; ++c)
                ws[8 * r + c] = ycc(k, byte_of(d, 3 * c), byte_of(d, 3 * c + 1), byte_of(d, 3 * c + 2)) - 128;
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint8_t* p = row + (int64_t)min(x0 + c, w - 1) * 3;
                ws[8 * r + c] = ycc(k, p[0], p[1], p[2]) - 128;
            }
        }
    }
}

// The 8x8 samples - 128 of chroma block (mx, my) of a 4:2:0 image
// (h2v2_downsample): chroma row cy is made of pixel rows 2cy and 2cy + 1, the
// second clamped to h - 1 (the row group is filled by repeating the last
// pixel row); chroma rows past ⌈h / 2⌉ repeat the last chroma row; pixel
// columns past w repeat the last; bias 1, 2, 1, 2, ... along the row.
__device__ __forceinline__ void load_h2v2(const uint8_t* __restrict__ img, int w, int h, int mx, int my, const Ycc& k,
                                          int (&ws)[64]) {
    const int x0 = mx * 16, crows = (h + 1) >> 1;
    const bool fast = x0 + 16 <= w;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int cy = min(my * 8 + r, crows - 1);
        int s[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) s[c] = 0;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const uint8_t* row = img + (int64_t)min(2 * cy + half, h - 1) * w * 3;
            if (fast) {
                uint32_t d[12];   // 48 B inside the row
#pragma unroll
                for (int i = 0; i < 12; ++i) d[i] = ld_u32_unaligned(row + (int64_t)x0 * 3 + 4 * i);
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    s[c >> 1] += ycc(k, byte_of(d, 3 * c), byte_of(d, 3 * c + 1), byte_of(d, 3 * c + 2));
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const uint8_t* p = row + (int64_t)min(x0 + c, w - 1) * 3;
                    s[c >> 1] += ycc(k, p[0], p[1], p[2]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) ws[8 * r + c] = ((s[c] + 1 + (c & 1)) >> 2) - 128;
    }
}

// jfdctint.c, one pass over eight values (CONST_BITS 13, PASS1_BITS 2).
template <bool FIRST>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int n = FIRST ? 11 : 15, rnd = 1 << (n - 1);
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
    int t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d0 = (t10 + t11) << 2;
        d4 = (t10 - t11) << 2;
    } else {
        d0 = (t10 + t11 + 2) >> 2;
        d4 = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    d2 = (z1 + t13 * 6270 + rnd) >> n;
    d6 = (z1 - t12 * 15137 + rnd) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    d7 = (t4 + z1 + z3 + rnd) >> n;
    d5 = (t5 + z2 + z4 + rnd) >> n;
    d3 = (t6 + z2 + z3 + rnd) >> n;
    d1 = (t7 + z1 + z4 + rnd) >> n;
}

// The AC codes of a block, in order: emit(bits, count) for each Huffman code
// with its magnitude bits appended (at most 16 + 10 bits), the ZRLs and the
// EOB.  get(k) is the coefficient at zigzag position k (k constant after
// unrolling); ac is the component's table in LDS.
template <class Get, class Emit>
__device__ __forceinline__ void walk_ac(Get&& get, const uint32_t* ac, Emit&& emit) {
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = get(k);
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            emit(ac[0xF0] >> 8, ac[0xF0] & 0xFFu);
            run -= 16;
        }
        const uint32_t nb = 32u - (uint32_t)__clz(v < 0 ? -v : v);
        const uint32_t e = ac[(run << 4) | nb];
        const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u);
        emit(((e >> 8) << nb) | mag, (e & 0xFFu) + nb);
        run = 0;
    }
    if (run) emit(ac[0] >> 8, ac[0] & 0xFFu);
}

// The DC code of a difference: (bits, count), at most 11 + 11 bits.
__device__ __forceinline__ void dc_code(int diff, const uint32_t* dc, uint32_t& bits, uint32_t& count) {
    const uint32_t nb = diff == 0 ? 0u : 32u - (uint32_t)__clz(diff < 0 ? -diff : diff);
    const uint32_t e = dc[nb];
    const uint32_t mag = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u);
    bits = ((e >> 8) << nb) | mag;
    count = (e & 0xFFu) + nb;
}

__device__ __forceinline__ void stage_huff(uint32_t (&s_ac)[2][256], uint32_t (&s_dc)[2][16]) {
    const uint32_t tid = threadIdx.x;
    s_ac[0][tid] = kHuff.ac[0][tid];
    s_ac[1][tid] = kHuff.ac[1][tid];
    if (tid < 32u) s_dc[tid >> 4][tid & 15u] = kHuff.dc[tid >> 4][tid & 15u];
    __syncthreads();
}

// Component of block j of an MCU, and the block before it of the same
// component in scan order (-1: none, the prediction is 0).
__device__ __forceinline__ int comp_of(const Geo& g, int j) { return g.sampling == IPP_JPEG_420 ? max(j - 3, 0) : j; }
__device__ __forceinline__ int pred_of(const Geo& g, int b, int m, int j) {
    if (g.sampling == IPP_JPEG_420 && j >= 1 && j <= 3) return b - 1;
    if (m == 0) return -1;
    return g.sampling == IPP_JPEG_420 && j == 0 ? b - 3 : b - g.bpm;
}

__global__ __launch_bounds__(kThreads) void k_jpeg_dct(const uint8_t* __restrict__ in, Geo g, QTab qt, Scratch sc) {
    __shared__ uint32_t s_ac[2][256], s_dc[2][16];
    stage_huff(s_ac, s_dc);
    const int m = (int)(blockIdx.x * kThreads + threadIdx.x), j = (int)blockIdx.y;   // j is block-uniform
    if (m >= g.nmcu) return;
    const int64_t image = blockIdx.z;
    const uint8_t* img = in + image * g.h * (int64_t)g.w * 3;
    const int my = (int)fdiv((uint32_t)m, g.dmcux), mx = m - my * g.mcux;
    const int c = comp_of(g, j), t = c == 0 ? 0 : 1;
    const Ycc k = ycc_of(c);
    int ws[64];
    bool dummy = false;
    if (g.sampling == IPP_JPEG_420 && j < 4) {
        int bx = 2 * mx + (j & 1), by = 2 * my + (j >> 1);
        // jccoefct.c: a block past the component's grid repeats the DC of the
        // block before it in the MCU — in a dummy bottom row that is Y01 (or
        // Y00 where Y01 is a dummy too), else its left neighbour.
        if (by >= g.hb) {
            dummy = true;
            by = 2 * my;
            bx = 2 * mx + 1 < g.wb ? 2 * mx + 1 : 2 * mx;
        } else if (bx >= g.wb) {
            dummy = true;
            bx -= 1;
        }
        load_full(img, g.w, g.h, bx, by, k, ws);
    } else if (g.sampling == IPP_JPEG_420) {
        load_h2v2(img, g.w, g.h, mx, my, k, ws);
    } else {
        load_full(img, g.w, g.h, mx, my, k, ws);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
        fdct8<true>(ws[8 * r], ws[8 * r + 1], ws[8 * r + 2], ws[8 * r + 3], ws[8 * r + 4], ws[8 * r + 5], ws[8 * r + 6],
                    ws[8 * r + 7]);
#pragma unroll
    for (int x = 0; x < 8; ++x)
        fdct8<false>(ws[x], ws[8 + x], ws[16 + x], ws[24 + x], ws[32 + x], ws[40 + x], ws[48 + x], ws[56 + x]);
    // coef / (8·q), halves away from zero
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int v = ws[i];
        const uint32_t e = qt.mq[t][i];   // scalar: t is block-uniform, i a constant
        const int q = (int)__umulhi(((uint32_t)(v < 0 ? -v : v) + 4u * (e & 0xFFu)) << 6, e >> 8);
        ws[i] = (dummy && i > 0) ? 0 : (v < 0 ? -q : q);
    }
    const int64_t b = image * g.nblk + (int64_t)m * g.bpm + j;
    uint32_t bits = 0u;
    walk_ac([&](int kk) { return ws[zz_nat(kk)]; }, s_ac[t], [&](uint32_t, uint32_t count) { bits += count; });
    sc.off[b] = bits;
    uint4* out = reinterpret_cast<uint4*>(sc.coef + b * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            p[e] = ((uint32_t)ws[zz_nat(8 * i + 2 * e)] & 0xFFFFu) | ((uint32_t)ws[zz_nat(8 * i + 2 * e + 1)] << 16);
        out[i] = make_uint4(p[0], p[1], p[2], p[3]);
    }
}

__global__ __launch_bounds__(kThreads) void k_jpeg_scan(Geo g, Scratch sc, int64_t capacity) {
    __shared__ uint64_t s_sum[kWaves];
    __shared__ uint32_t s_ac[2][256], s_dc[2][16];
    stage_huff(s_ac, s_dc);
    const int64_t image = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int16_t* coef = sc.coef + image * g.nblk * 64;
    uint64_t* off = sc.off + image * g.nblk;
    uint64_t carry = 0;
    for (int base = 0; base < g.nblk; base += kScanStep) {
        uint32_t len[kScanPerThread];
        uint64_t mine = 0;
#pragma unroll
        for (int e = 0; e < kScanPerThread; ++e) {
            const int b = base + (int)tid * kScanPerThread + e;
            len[e] = 0u;
            if (b < g.nblk) {
                const int m = b / g.bpm, j = b - m * g.bpm;
                const int p = pred_of(g, b, m, j);
                const int diff = (int)coef[(int64_t)b * 64] - (p < 0 ? 0 : (int)coef[(int64_t)p * 64]);
                uint32_t bits, count;
                dc_code(diff, s_dc[comp_of(g, j) == 0 ? 0 : 1], bits, count);
                len[e] = (uint32_t)off[b] + count;
            }
            mine += len[e];
        }
        uint64_t inc = mine;   // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t up = __shfl_up(inc, o);
            if (lane >= (uint32_t)o) inc += up;
        }
        if (lane == 63u) s_sum[wave] = inc;
        __syncthreads();
        uint64_t before = carry, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kWaves; ++k) {
            if (k < wave) before += s_sum[k];
            all += s_sum[k];
        }
        uint64_t at = before + inc - mine;
#pragma unroll
        for (int e = 0; e < kScanPerThread; ++e) {
            const int b = base + (int)tid * kScanPerThread + e;
            if (b < g.nblk) off[b] = at;
            at += len[e];
        }
        carry += all;
        __syncthreads();   // s_sum is rewritten by the next step
    }
    if (tid == 0u) {
        Rec r;
        r.bits = carry;
        r.status = (carry + 7u) / 8u > (uint64_t)capacity ? (uint32_t)IPP_JPEG_OVERFLOW : 0u;
        r.pad_ = 0u;
        sc.rec[image] = r;
    }
}

__global__ __launch_bounds__(kThreads) void k_jpeg_zero(Scratch sc) {
    const int64_t image = blockIdx.y;
    const Rec r = sc.rec[image];
    const int64_t at = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 16;
    // through the 16 B that hold the last bit (raw_pitch is 16 B past the capacity's pitch)
    if (r.status != 0u || at >= sc.raw_pitch || (uint64_t)at * 8u > r.bits) return;
    *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(sc.raw) + image * sc.raw_pitch + at) = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kThreads) void k_jpeg_write(Geo g, Scratch sc) {
    __shared__ uint32_t s_ac[2][256], s_dc[2][16];
    stage_huff(s_ac, s_dc);
    const int b = (int)(blockIdx.x * kThreads + threadIdx.x);
    const int64_t image = blockIdx.y;
    if (b >= g.nblk || sc.rec[image].status != 0u) return;
    const int16_t* coef = sc.coef + image * g.nblk * 64;
    const int m = b / g.bpm, j = b - m * g.bpm, t = comp_of(g, j) == 0 ? 0 : 1;
    const int p = pred_of(g, b, m, j);
    uint4 c[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) c[i] = reinterpret_cast<const uint4*>(coef + (int64_t)b * 64)[i];
    auto get = [&](int k) {
        const uint4& q = c[k >> 3];
        const uint32_t d = ((k >> 1) & 3) == 0 ? q.x : ((k >> 1) & 3) == 1 ? q.y : ((k >> 1) & 3) == 2 ? q.z : q.w;
        return (int)(int16_t)(uint16_t)((k & 1) ? d >> 16 : d & 0xFFFFu);
    };
    const uint64_t pos = sc.off[image * g.nblk + b];
    uint32_t* raw = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(sc.raw) + image * sc.raw_pitch);
    const int64_t nwords = sc.raw_pitch / 4;
    int64_t wi = (int64_t)(pos >> 5);
    uint32_t fill = (uint32_t)pos & 31u;   // bits of word wi that precede this block's (and then: that are pending in acc)
    uint64_t acc = 0;                       // pending bits, from bit 63 down; bit position p of the stream is bit 31 - (p & 31) of word p >> 5
    bool first = true;
    auto put = [&](uint32_t bits, uint32_t count) {   // fill < 32, count <= 26
        acc |= (uint64_t)bits << (64u - fill - count);
        fill += count;
        if (fill >= 32u) {
            const uint32_t wd = (uint32_t)(acc >> 32);
            if (wi < nwords) {
                if (first) atomicOr(raw + wi, wd);   // may hold the end of the blocks before
                else raw[wi] = wd;                   // wholly this block's
            }
            first = false;
            acc <<= 32, fill -= 32u, ++wi;
        }
    };
    uint32_t bits, count;
    dc_code(get(0) - (p < 0 ? 0 : (int)coef[(int64_t)p * 64]), s_dc[t], bits, count);
    put(bits, count);
    walk_ac(get, s_ac[t], put);
    if (fill > 0u && wi < nwords) {
        const uint32_t wd = (uint32_t)(acc >> 32);
        if (wd != 0u) atomicOr(raw + wi, wd);   // may hold the start of the blocks after
    }
}

// Byte e (0..15, stream order) of 16 B of the unstuffed stream starting at
// byte `at`; the last byte of the scan is filled with 1-bits.
__device__ __forceinline__ uint32_t stream_byte(const uint4& v, int e, int64_t at, int64_t nbytes, uint64_t bits) {
    const uint32_t wd = (e >> 2) == 0 ? v.x : (e >> 2) == 1 ? v.y : (e >> 2) == 2 ? v.z : v.w;
    uint32_t x = (wd >> (24 - 8 * (e & 3))) & 0xFFu;
    if (at + e == nbytes - 1 && (bits & 7u) != 0u) x |= 0xFFu >> (bits & 7u);
    return x;
}

// The thread's 16 B (zeros past the stream) and the number of 0xFF among them.
__device__ __forceinline__ uint32_t load_ff(const Scratch& sc, int64_t image, const Rec& r, int64_t at, int64_t nbytes,
                                            uint4& v) {
    v = make_uint4(0u, 0u, 0u, 0u);
    if (at >= nbytes) return 0u;
    v = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(sc.raw) + image * sc.raw_pitch + at);
    uint32_t n = 0u;
#pragma unroll
    for (int e = 0; e < 16; ++e) n += (at + e < nbytes && stream_byte(v, e, at, nbytes, r.bits) == 0xFFu) ? 1u : 0u;
    return n;
}

__global__ __launch_bounds__(kThreads) void k_jpeg_ffcount(Scratch sc) {
    __shared__ uint32_t s_n[kWaves];
    const int64_t image = blockIdx.y;
    const Rec r = sc.rec[image];
    const int64_t nbytes = (int64_t)((r.bits + 7u) / 8u);
    if (r.status != 0u || (int64_t)blockIdx.x * kChunk >= nbytes) return;   // block-uniform
    uint4 v;
    uint32_t n = load_ff(sc, image, r, ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 16, nbytes, v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63u) == 0u) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t all = 0u;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) all += s_n[k];
        sc.ff[image * sc.nchunk + blockIdx.x] = all;
    }
}

// Exclusive sum of 256 values across the workgroup; `all` receives the total.
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

__global__ __launch_bounds__(kThreads) void k_jpeg_ffscan(Scratch sc, int64_t capacity, int32_t* __restrict__ hdr) {
    __shared__ uint32_t s_sum[kWaves];
    const int64_t image = blockIdx.x;
    const Rec r = sc.rec[image];
    const int64_t nbytes = (int64_t)((r.bits + 7u) / 8u);
    int32_t* h = hdr + IPP_JPEG_HDR * image;
    if (r.status != 0u) {   // block-uniform: the unstuffed stream alone is too long
        if (threadIdx.x == 0u) h[0] = (int32_t)min(nbytes, (int64_t)INT32_MAX), h[1] = (int32_t)r.status;
        return;
    }
    uint32_t* ff = sc.ff + image * sc.nchunk;
    const int used = (int)((nbytes + kChunk - 1) / kChunk);
    uint32_t carry = 0u;
    for (int base = 0; base < used; base += kThreads) {
        const int k = base + (int)threadIdx.x;
        const uint32_t v = k < used ? ff[k] : 0u;
        uint32_t all;
        const uint32_t ex = block_exclusive(v, s_sum, all);
        if (k < used) ff[k] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0u) {
        const int64_t stuffed = nbytes + carry;
        h[0] = (int32_t)min(stuffed, (int64_t)INT32_MAX);
        h[1] = stuffed > capacity ? IPP_JPEG_OVERFLOW : 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_jpeg_stuff(Scratch sc, const int32_t* __restrict__ hdr,
                                                         uint8_t* __restrict__ slots, int64_t slot_pitch) {
    __shared__ uint32_t s_sum[kWaves];
    const int64_t image = blockIdx.y;
    const Rec r = sc.rec[image];
    const int64_t nbytes = (int64_t)((r.bits + 7u) / 8u);
    if (hdr[IPP_JPEG_HDR * image + 1] != 0 || (int64_t)blockIdx.x * kChunk >= nbytes) return;   // block-uniform
    const int64_t total = hdr[IPP_JPEG_HDR * image];
    const int64_t at = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 16;
    uint4 v;
    const uint32_t n = load_ff(sc, image, r, at, nbytes, v);
    uint32_t all;
    const uint32_t ex = block_exclusive(n, s_sum, all);
    if (at >= nbytes) return;
    uint8_t* out = slots + image * slot_pitch;
    int64_t pos = at + sc.ff[image * sc.nchunk + blockIdx.x] + ex;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const uint32_t x = stream_byte(v, e, at, nbytes, r.bits);
        if (at + e < nbytes) {
            if (pos < total) out[pos] = (uint8_t)x;
            ++pos;
            if (x == 0xFFu) {
                if (pos < total) out[pos] = 0u;
                ++pos;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_jpeg_pack(const uint8_t* __restrict__ slots, int64_t slot_pitch,
                                                        const int32_t* __restrict__ hdr,
                                                        const int64_t* __restrict__ offsets, uint8_t* __restrict__ out) {
    const int64_t image = blockIdx.y;
    const int64_t nbytes = hdr[IPP_JPEG_HDR * image + 1] != 0 ? 0 : hdr[IPP_JPEG_HDR * image];
    const int64_t at = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (at >= nbytes || at >= slot_pitch) return;
    const uint8_t* src = slots + image * slot_pitch + at;   // 16-B aligned, 16 B inside the slot's pitch
    uint8_t* dst = out + offsets[image] + at;
    const int n = (int)min((int64_t)16, nbytes - at);
    uint32_t wd[4];
    load16(src, 16, true, wd);
    store16(dst, n, n == 16 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0, wd);
}

int check_shape(int32_t n, int32_t w, int32_t h, int32_t sampling, int64_t capacity) {
    if (n < 0 || n > kMaxImages || w < 1 || h < 1 || w > IPP_JPEG_MAX_SIDE || h > IPP_JPEG_MAX_SIDE) return IPP_E_ARG;
    if (sampling != IPP_JPEG_420 && sampling != IPP_JPEG_444) return IPP_E_ARG;
    if (capacity < 1 || capacity > IPP_JPEG_MAX_CAPACITY) return IPP_E_ARG;
    return IPP_OK;
}

}  // namespace

extern "C" int64_t ipp_jpeg_scratch_bytes(int32_t n_images, int32_t w, int32_t h, int32_t sampling, int64_t capacity) {
    if (check_shape(n_images, w, h, sampling, capacity) != IPP_OK) return IPP_E_ARG;
    return scratch_of(nullptr, n_images, geo_of(w, h, sampling), capacity).total;
}

extern "C" int ipp_jpeg_encode(const uint8_t* in, int32_t n_images, int32_t w, int32_t h, int32_t sampling,
                               const uint16_t* qtab, uint8_t* scratch, uint8_t* slots, int64_t capacity, int32_t* hdr,
                               void* stream) {
    if (!in || !qtab || !scratch || !slots || !hdr) return IPP_E_ARG;
    if (check_shape(n_images, w, h, sampling, capacity) != IPP_OK) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(slots)) & 15u) != 0 ||
        (reinterpret_cast<uintptr_t>(hdr) & 3u) != 0)
        return IPP_E_ARG;
    QTab qt;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const uint32_t q = qtab[64 * t + i];
            if (q < 1u || q > 255u) return IPP_E_ARG;
            qt.mq[t][i] = (((1u << 26) / (8u * q) + 1u) << 8) | q;
        }
    if (n_images == 0) return IPP_OK;
    hipStream_t s = (hipStream_t)stream;
    const Geo g = geo_of(w, h, sampling);
    const Scratch sc = scratch_of(scratch, n_images, g, capacity);
    const uint32_t n = (uint32_t)n_images;
    hipLaunchKernelGGL(k_jpeg_dct, dim3((uint32_t)((g.nmcu + kThreads - 1) / kThreads), (uint32_t)g.bpm, n),
                       dim3(kThreads), 0, s, in, g, qt, sc);
    hipLaunchKernelGGL(k_jpeg_scan, dim3(n), dim3(kThreads), 0, s, g, sc, capacity);
    hipLaunchKernelGGL(k_jpeg_zero, dim3((uint32_t)sc.nchunk, n), dim3(kThreads), 0, s, sc);
    hipLaunchKernelGGL(k_jpeg_write, dim3((uint32_t)((g.nblk + kThreads - 1) / kThreads), n), dim3(kThreads), 0, s, g,
                       sc);
    hipLaunchKernelGGL(k_jpeg_ffcount, dim3((uint32_t)sc.nchunk, n), dim3(kThreads), 0, s, sc);
    hipLaunchKernelGGL(k_jpeg_ffscan, dim3(n), dim3(kThreads), 0, s, sc, capacity, hdr);
    hipLaunchKernelGGL(k_jpeg_stuff, dim3((uint32_t)sc.nchunk, n), dim3(kThreads), 0, s, sc, hdr, slots,
                       pitch16(capacity));
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_jpeg_pack(const uint8_t* slots, int64_t capacity, const int32_t* hdr, int32_t n_images,
                             const int64_t* offsets, uint8_t* out, void* stream) {
    if (!slots || !hdr || !offsets || !out || n_images < 0 || n_images > kMaxImages) return IPP_E_ARG;
    if (capacity < 1 || capacity > IPP_JPEG_MAX_CAPACITY) return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(slots) & 15u) != 0 || (reinterpret_cast<uintptr_t>(hdr) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(offsets) & 7u) != 0)
        return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    const int64_t pitch = pitch16(capacity);
    hipLaunchKernelGGL(k_jpeg_pack, dim3((uint32_t)((pitch + kChunk - 1) / kChunk), (uint32_t)n_images), dim3(kThreads),
                       0, (hipStream_t)stream, slots, pitch, hdr, offsets, out);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}
