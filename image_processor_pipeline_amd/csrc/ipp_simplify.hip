// Douglas–Peucker simplification of the packed scene polygons on the device
// (ipp.h: ipp_polygons_simplify, ipp_polygons_simplify_pack; the rule — anchors,
// the split of a segment, its ties, the triangle floor — is stated there in
// exact integers and in DESIGN.md §3).
//
//   k_simplify       one workgroup per ring, level by level: every open vertex
//                    carries its segment (a, b); a round offers (measure, ~j) to
//                    the segment's 64-bit slot by integer atomicMax, and after a
//                    barrier every vertex of the segment reads the winner, tests
//                    it against eps_q and becomes kept, moves to the left or the
//                    right half, or is dropped with its closed segment.  A ring
//                    of at most IPP_SIMPLIFY_LDS_VERTS vertices keeps its points
//                    and per-vertex state in LDS; a longer one runs the same
//                    loop on the arrays of the global scratch.  Then a block
//                    scan of the keep flags: mark = 1 + position among the kept.
//   k_simplify_pack  one workgroup per ring: the marked vertices to their places.
// No kernel waits on another block; the only atomics are integer max, whose
// result does not depend on their order.
//
// Slots are written once and never cleared between rounds.  Segment (a, b)
// offers to slot a when it is a root chain or a right half (a was kept in the
// round that made it), and to slot b − 1 when it is a left half (b was kept in
// that round).  Only a segment with an interior vertex offers, so slot b − 1 is
// an interior vertex of a left half: never kept so far, hence never a right
// half's slot, and its right neighbour b was not kept before, hence never a
// left half's slot.  A right half's slot a was interior until this round, so
// no right half used it, and a left half that used it ended at a + 1: were that
// this segment's b, it would have no interior vertex.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ipp.h"
#include "ipp_device.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = IPP_SIMPLIFY_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kLdsVerts = IPP_SIMPLIFY_LDS_VERTS;
constexpr uint32_t kClosed = 0xFFFFFFFFu;  // in a[]: the vertex is settled, b[] = 1 kept / 0 dropped
constexpr uint32_t kLeft = 0x80000000u;    // in b[]: the segment is a left half (its slot is b − 1)
constexpr int kMaxCoord = 16384, kMaxEpsQ = 4096;
constexpr int64_t kMaxImages = 1 << 24;    // n_images · 256 threads stays below 2^32

inline int64_t mark_bytes(int64_t total) { return (total * 4 + 255) / 256 * 256; }

// A ring in LDS: points packed (x | y << 16, both <= 16384) and the per-vertex state.
struct LdsRing {
    uint32_t *xy, *a, *b;
    u64* slot;
    __device__ __forceinline__ int2 pt(uint32_t j) const {
        const uint32_t v = xy[j];
        return make_int2((int)(v & 0xFFFFu), (int)(v >> 16));
    }
    __device__ __forceinline__ u64 winner(uint32_t s) const { return slot[s]; }
};

// A ring too long for LDS: points from the packed buffer, state in the scratch.
// a[j] and b[j] are only ever touched by the thread that owns j; the slots are
// written by atomics (at the L2) and read past the L1 for that reason.
struct GlobalRing {
    const int32_t* v;
    uint32_t *a, *b;
    u64* slot;
    __device__ __forceinline__ int2 pt(uint32_t j) const { return make_int2(v[2 * (int64_t)j], v[2 * (int64_t)j + 1]); }
    __device__ __forceinline__ u64 winner(uint32_t s) const {
        return __hip_atomic_load(slot + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

struct Shared {
    u64 best;
    uint32_t wave[kWaves];
};

__device__ __forceinline__ u64 wave_max(u64 k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(k, o);
        k = t > k ? t : k;
    }
    return k;
}

// Block-wide max of the threads' keys through sh.best (0 = none).  Ends on a barrier.
__device__ __forceinline__ u64 block_max(Shared& sh, u64 k) {
    if (threadIdx.x == 0) sh.best = 0ull;
    __syncthreads();
    k = wave_max(k);
    if ((threadIdx.x & 63) == 0 && k != 0ull) atomicMax(&sh.best, k);
    __syncthreads();
    return sh.best;
}

__device__ __forceinline__ uint32_t abs_cross(int2 pa, int2 pb, int2 pj) {
    const int c = (pb.x - pa.x) * (pj.y - pa.y) - (pb.y - pa.y) * (pj.x - pa.x);  // |.| <= 2^29
    return (uint32_t)(c < 0 ? -c : c);
}
__device__ __forceinline__ uint32_t dist2(int2 p, int2 q) {
    const int dx = p.x - q.x, dy = p.y - q.y;
    return (uint32_t)(dx * dx + dy * dy);  // <= 2^29
}

template <class Ring>
__device__ __forceinline__ void simplify_ring(const Ring& R, uint32_t n, uint32_t eps2, uint32_t* __restrict__ mark,
                                              int32_t* __restrict__ count, Shared& sh) {
    const uint32_t tid = threadIdx.x;
    // anchor B: the farthest vertex from P[0], ties to the least index
    const int2 p0 = R.pt(0);
    u64 k = 0ull;
    for (uint32_t j = tid; j < n; j += kThreads)
        if (j >= 1) {
            const u64 key = ((u64)dist2(R.pt(j), p0) << 32) | (uint32_t)~j;
            k = key > k ? key : k;
        }
    const uint32_t B = ~(uint32_t)block_max(sh, k);
    // the two chains (0, B) and (B, n); every other vertex is interior to one of them
    for (uint32_t j = tid; j < n; j += kThreads) {
        const bool anchor = j == 0 || j == B;
        R.a[j] = anchor ? kClosed : j < B ? 0u : B;
        R.b[j] = anchor ? 1u : j < B ? B : n;
        R.slot[j] = 0ull;
    }
    __syncthreads();
    for (;;) {
        for (uint32_t j = tid; j < n; j += kThreads) {
            const uint32_t a = R.a[j];
            if (a == kClosed) continue;
            const uint32_t bf = R.b[j], b = bf & ~kLeft, s = (bf & kLeft) ? b - 1u : a;
            const int2 pa = R.pt(a), pb = R.pt(b == n ? 0u : b), pj = R.pt(j);
            const uint32_t m = dist2(pb, pa) ? abs_cross(pa, pb, pj) : dist2(pj, pa);
            atomicMax(R.slot + s, ((u64)m << 32) | (uint32_t)~j);
        }
        __syncthreads();
        bool open = false;
        for (uint32_t j = tid; j < n; j += kThreads) {
            const uint32_t a = R.a[j];
            if (a == kClosed) continue;
            const uint32_t bf = R.b[j], b = bf & ~kLeft, s = (bf & kLeft) ? b - 1u : a;
            const u64 w = R.winner(s);
            const uint32_t c = ~(uint32_t)w;
            const u64 m = w >> 32;
            const u64 len2 = dist2(R.pt(b == n ? 0u : b), R.pt(a));
            // 16·cross² <= 2^60 and eps_q²·len2 <= 2^53; with len2 = 0, m is a squared distance <= 2^29
            const bool split = len2 ? 16ull * m * m > (u64)eps2 * len2 : 16ull * m > (u64)eps2;
            if (!split) {
                R.a[j] = kClosed, R.b[j] = 0u;
            } else if (j == c) {
                R.a[j] = kClosed, R.b[j] = 1u;
            } else if (j < c) {
                R.b[j] = c | kLeft, open = true;
            } else {
                R.a[j] = c, R.b[j] = b, open = true;
            }
        }
        if (!__syncthreads_or(open)) break;
    }
    // mark = 1 + the vertex's position among the kept
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += kThreads) {
        const uint32_t j = c0 + tid;
        const bool kept = j < n && R.b[j] == 1u;  // (every vertex is settled: b is 1 or 0)
        const u64 m = __ballot(kept);
        if ((tid & 63) == 0) sh.wave[tid >> 6] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = base, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            before += w < (int)(tid >> 6) ? sh.wave[w] : 0u;
            all += sh.wave[w];
        }
        if (j < n) mark[j] = kept ? before + (uint32_t)__popcll(m & ((1ull << (tid & 63)) - 1ull)) + 1u : 0u;
        base += all;
        __syncthreads();
    }
    // at least a triangle: with the anchors alone, the vertex farthest from the line (A, B), if off it
    if (base == 2) {
        const int2 pB = R.pt(B);
        k = 0ull;
        for (uint32_t j = tid; j < n; j += kThreads) {
            const u64 key = ((u64)abs_cross(p0, pB, R.pt(j)) << 32) | (uint32_t)~j;
            k = key > k ? key : k;
        }
        const u64 w = block_max(sh, k);
        if ((w >> 32) != 0ull) {
            const uint32_t c = ~(uint32_t)w;
            if (tid == 0) mark[c] = c < B ? 2u : 3u, mark[B] = c < B ? 3u : 2u;
            base = 3;
        }
    }
    if (tid == 0) *count = (int32_t)base;
}

__global__ __launch_bounds__(kThreads) void k_simplify(const int32_t* __restrict__ verts,
                                                       const int64_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ hdr, uint32_t eps2,
                                                       uint32_t* __restrict__ marks, u64* __restrict__ g_slot,
                                                       uint32_t* __restrict__ g_a, uint32_t* __restrict__ g_b,
                                                       int32_t* __restrict__ counts) {
    __shared__ u64 s_slot[kLdsVerts];
    __shared__ uint32_t s_xy[kLdsVerts], s_a[kLdsVerts], s_b[kLdsVerts];
    __shared__ Shared sh;
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    const int32_t* h = hdr + (int64_t)IPP_CONTOUR_HDR * i;
    if (h[3] <= 0 || h[7] != 0) {  // block-uniform
        if (tid == 0) counts[i] = 0;
        return;
    }
    const uint32_t n = (uint32_t)h[3];
    const int64_t off = offsets[i];
    const int32_t* v = verts + 2 * off;
    uint32_t* mark = marks + off;
    if (n < 3) {  // returned whole
        for (uint32_t j = tid; j < n; j += kThreads) mark[j] = j + 1u;
        if (tid == 0) counts[i] = (int32_t)n;
        return;
    }
    if (n <= kLdsVerts) {
        for (uint32_t j = tid; j < n; j += kThreads)
            s_xy[j] = ((uint32_t)v[2 * j] & 0xFFFFu) | ((uint32_t)v[2 * j + 1] << 16);
        __syncthreads();
        simplify_ring(LdsRing{s_xy, s_a, s_b, s_slot}, n, eps2, mark, counts + i, sh);
    } else {
        simplify_ring(GlobalRing{v, g_a + off, g_b + off, g_slot + off}, n, eps2, mark, counts + i, sh);
    }
}

__global__ __launch_bounds__(kThreads) void k_simplify_pack(const int32_t* __restrict__ verts,
                                                            const int64_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ hdr,
                                                            const uint32_t* __restrict__ marks,
                                                            const int32_t* __restrict__ counts,
                                                            const int64_t* __restrict__ out_offsets,
                                                            int32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x;
    const int32_t* h = hdr + (int64_t)IPP_CONTOUR_HDR * i;
    if (h[3] <= 0 || h[7] != 0 || counts[i] <= 0) return;
    const uint32_t n = (uint32_t)h[3], kept = (uint32_t)counts[i];
    const int64_t off = offsets[i];
    int32_t* o = out + 2 * out_offsets[i];
    for (uint32_t j = threadIdx.x; j < n; j += kThreads) {
        const uint32_t r = marks[off + j];
        if (r == 0u || r > kept) continue;
        o[2 * (int64_t)(r - 1u)] = verts[2 * (off + j)];
        o[2 * (int64_t)(r - 1u) + 1] = verts[2 * (off + j) + 1];
    }
}

}  // namespace

extern "C" int64_t ipp_polygons_simplify_scratch_bytes(int32_t n_images, int64_t total_vertices) {
    if (n_images < 0 || n_images >= kMaxImages || total_vertices < 0 || total_vertices > (1ll << 40)) return IPP_E_ARG;
    return mark_bytes(total_vertices) + 16 * total_vertices;
}

extern "C" int ipp_polygons_simplify(const int32_t* verts, const int64_t* offsets, const int32_t* hdr,
                                     int32_t n_images, int64_t total_vertices, int32_t bg_w, int32_t bg_h,
                                     int32_t eps_q, uint8_t* scratch, int32_t* counts, void* stream) {
    if (!verts || !offsets || !hdr || !scratch || !counts) return IPP_E_ARG;
    if (n_images < 0 || n_images >= kMaxImages || total_vertices < 0 || total_vertices > (1ll << 40)) return IPP_E_ARG;
    if (eps_q < 1 || eps_q > kMaxEpsQ) return IPP_E_ARG;
    if (bg_w < 1 || bg_w > kMaxCoord || bg_h < 1 || bg_h > kMaxCoord) return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15u) != 0) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(verts) | reinterpret_cast<uintptr_t>(hdr) | reinterpret_cast<uintptr_t>(counts)) &
         3u) != 0 ||
        (reinterpret_cast<uintptr_t>(offsets) & 7u) != 0)
        return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    uint32_t* marks = reinterpret_cast<uint32_t*>(scratch);
    u64* slot = reinterpret_cast<u64*>(scratch + mark_bytes(total_vertices));
    uint32_t* a = reinterpret_cast<uint32_t*>(slot + total_vertices);
    uint32_t* b = a + total_vertices;
    hipLaunchKernelGGL(k_simplify, dim3((uint32_t)n_images), dim3(kThreads), 0, (hipStream_t)stream, verts, offsets,
                       hdr, (uint32_t)(eps_q * eps_q), marks, slot, a, b, counts);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}

extern "C" int ipp_polygons_simplify_pack(const int32_t* verts, const int64_t* offsets, const int32_t* hdr,
                                          const uint8_t* scratch, const int32_t* counts, const int64_t* out_offsets,
                                          int32_t n_images, int32_t* out, void* stream) {
    if (!verts || !offsets || !hdr || !scratch || !counts || !out_offsets || !out) return IPP_E_ARG;
    if (n_images < 0 || n_images >= kMaxImages) return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15u) != 0) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(verts) | reinterpret_cast<uintptr_t>(hdr) | reinterpret_cast<uintptr_t>(counts) |
          reinterpret_cast<uintptr_t>(out)) &
         3u) != 0 ||
        ((reinterpret_cast<uintptr_t>(offsets) | reinterpret_cast<uintptr_t>(out_offsets)) & 7u) != 0)
        return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    hipLaunchKernelGGL(k_simplify_pack, dim3((uint32_t)n_images), dim3(kThreads), 0, (hipStream_t)stream, verts,
                       offsets, hdr, reinterpret_cast<const uint32_t*>(scratch), counts, out_offsets, out);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}
