// Oriented boxes (YOLO-OBB) of the packed scene polygons on the device
// (ipp.h: ipp_polygons_obb; the rule — the canonical strictly convex hull, the
// rectangle on an edge, the exact choice and its ties, the record — is stated
// there in exact integers and in DESIGN.md §3).
//
//   k_obb_rings  one workgroup per ring, three phases:
//     rows    the ring's least and greatest y, then per lattice row the least
//             and the greatest x by integer atomicMin / atomicMax in LDS, a
//             window of IPP_OBB_LDS_ROWS rows at a time (a taller ring sweeps
//             its vertices once per window);
//     chain   after each window one lane of wave 0 extends the right chain
//             (first point, then every row's greatest x; turns stay > 0) and
//             one lane of wave 1 the left chain (every row's least x, and the
//             last row's greatest; turns stay < 0) over the window's rows in
//             increasing y: Andrew's monotone chain on at most two points per
//             row.  The first IPP_OBB_LDS_HULL points of a chain live in LDS,
//             the rest in the ring's own slots of the global scratch.  The
//             hull is the right chain followed by the left one reversed
//             without its ends;
//     search  thread t takes hull edges t, t + 256, ...: lo, hi and hgt over
//             the hull's vertices (a linear form over a point set has its
//             extremes at hull vertices), the least area by the cross-
//             multiplied 128-bit comparison, ties to the lesser edge; a
//             shuffle reduction per wave, then one thread writes the record.
// Coordinates are clamped to 0..16384 on load: vertices outside the contract
// give an unspecified record but neither an access out of bounds nor more than
// ⌈16385 / IPP_OBB_LDS_ROWS⌉ windows.  No kernel waits on another block; the
// only atomics are integer min and max, whose result does not depend on their
// order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ipp.h"
#include "ipp_device.h"

namespace {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int kThreads = IPP_OBB_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kRows = IPP_OBB_LDS_ROWS;
constexpr uint32_t kHull = IPP_OBB_LDS_HULL;
constexpr int kMaxCoord = 16384;
constexpr int64_t kMaxImages = 1 << 24;    // n_images · 256 threads stays below 2^32
constexpr uint32_t kNone = 0xFFFFFFFFu;

inline int64_t chain_bytes(int64_t total) { return (total * 8 + 255) / 256 * 256; }

// A point packed x | y << 16, both clamped to 0..16384.
__device__ __forceinline__ uint32_t load_pt(const int32_t* __restrict__ v, uint32_t j) {
    const int x = min(max(v[2 * (int64_t)j], 0), kMaxCoord), y = min(max(v[2 * (int64_t)j + 1], 0), kMaxCoord);
    return (uint32_t)x | ((uint32_t)y << 16);
}
__device__ __forceinline__ int px(uint32_t p) { return (int)(p & 0xFFFFu); }
__device__ __forceinline__ int py(uint32_t p) { return (int)(p >> 16); }

// One monotone chain: entries below kHull in LDS, the others in the ring's slots of the scratch.  The lane
// that builds it keeps its size and its two topmost points in registers.
struct Chain {
    uint32_t* lds;
    uint32_t* glb;
    uint32_t sz, top, below;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return i < kHull ? lds[i] : glb[i - kHull]; }
    // for the other threads of the block, after the builder's fence and a barrier
    __device__ __forceinline__ uint32_t shared(uint32_t i) const {
        return i < kHull ? lds[i] : __hip_atomic_load(glb + (i - kHull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // append p, first dropping every top that does not turn by sign·cross > 0
    __device__ __forceinline__ void push(uint32_t p, int sign) {
        while (sz >= 2u) {
            const int ux = px(top) - px(below), uy = py(top) - py(below);
            const int vx = px(p) - px(top), vy = py(p) - py(top);
            if (sign * (ux * vy - uy * vx) > 0) break;  // |cross| <= 2^29
            --sz;
            top = below;
            if (sz >= 2u) below = get(sz - 2u);
        }
        if (sz < kHull)
            lds[sz] = p;
        else
            glb[sz - kHull] = p;
        below = top;
        top = p;
        ++sz;
    }
};

// The rectangle on one hull edge; e == kNone: none.
struct Cand {
    uint32_t e, nn, hgt;
    int32_t lo, hi;
};

__device__ __forceinline__ bool beats(const Cand& c1, const Cand& c2) {
    if (c1.e == kNone) return false;
    if (c2.e == kNone) return true;
    // (hi − lo)·hgt <= 2^59, times nn <= 2^29: 128 bits
    const u128 l = (u128)((u64)(uint32_t)(c1.hi - c1.lo) * c1.hgt) * c2.nn;
    const u128 r = (u128)((u64)(uint32_t)(c2.hi - c2.lo) * c2.hgt) * c1.nn;
    return l < r || (l == r && c1.e < c2.e);
}

struct Shared {
    int ymin, ymax;
    uint32_t na, nb;
    Cand wave[kWaves];
};

__global__ __launch_bounds__(kThreads) void k_obb_rings(const int32_t* __restrict__ verts,
                                                        const int64_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ hdr,
                                                        uint32_t* __restrict__ g_chain, int64_t total,
                                                        int32_t* __restrict__ obb) {
    __shared__ int s_min[kRows], s_max[kRows];
    __shared__ uint32_t s_a[kHull], s_b[kHull];
    __shared__ Shared sh;
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    const int32_t* h = hdr + (int64_t)IPP_CONTOUR_HDR * i;
    int32_t* rec = obb + (int64_t)IPP_OBB_REC * i;
    if (h[3] <= 0 || h[7] != 0) {  // block-uniform
        if (tid < (uint32_t)IPP_OBB_REC) rec[tid] = 0;
        return;
    }
    const uint32_t n = (uint32_t)h[3];
    const int64_t off = offsets[i];
    const int32_t* v = verts + 2 * off;

    // rows: the ring's y range
    if (tid == 0) sh.ymin = INT_MAX, sh.ymax = INT_MIN;
    __syncthreads();
    int y0 = INT_MAX, y1 = INT_MIN;
    for (uint32_t j = tid; j < n; j += kThreads) {
        const int y = py(load_pt(v, j));
        y0 = min(y0, y), y1 = max(y1, y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) y0 = min(y0, __shfl_xor(y0, o)), y1 = max(y1, __shfl_xor(y1, o));
    if ((tid & 63u) == 0) atomicMin(&sh.ymin, y0), atomicMax(&sh.ymax, y1);
    __syncthreads();
    const int ymin = sh.ymin, ymax = sh.ymax;

    // rows and chain, a window of kRows rows at a time
    Chain A{s_a, g_chain + off, 0u, 0u, 0u}, B{s_b, g_chain + total + off, 0u, 0u, 0u};
    for (int wy = ymin; wy <= ymax; wy += (int)kRows) {
        const uint32_t rows = min(kRows, (uint32_t)(ymax - wy + 1));
        for (uint32_t r = tid; r < rows; r += kThreads) s_min[r] = INT_MAX, s_max[r] = INT_MIN;
        __syncthreads();
        for (uint32_t j = tid; j < n; j += kThreads) {
            const uint32_t p = load_pt(v, j), r = (uint32_t)(py(p) - wy);
            if (r < rows) atomicMin(&s_min[r], px(p)), atomicMax(&s_max[r], px(p));
        }
        __syncthreads();
        if (tid == 0) {
            for (uint32_t r = 0; r < rows; ++r) {
                const int mn = s_min[r];
                if (mn == INT_MAX) continue;
                const int mx = s_max[r];
                const uint32_t yy = (uint32_t)(wy + (int)r) << 16;
                if (A.sz == 0u) {
                    A.push((uint32_t)mn | yy, 1);
                    if (mx != mn) A.push((uint32_t)mx | yy, 1);
                } else {
                    A.push((uint32_t)mx | yy, 1);
                }
            }
        } else if (tid == 64) {
            for (uint32_t r = 0; r < rows; ++r) {
                const int mn = s_min[r];
                if (mn == INT_MAX) continue;
                const int mx = s_max[r];
                const uint32_t yy = (uint32_t)(wy + (int)r) << 16;
                B.push((uint32_t)mn | yy, -1);
                if (wy + (int)r == ymax && mx != mn) B.push((uint32_t)mx | yy, -1);
            }
        }
        __syncthreads();
    }
    if (tid == 0) sh.na = A.sz;
    if (tid == 64) sh.nb = B.sz;
    __threadfence();  // the chains' entries in the scratch, before the other threads read them
    __syncthreads();
    const uint32_t na = sh.na, nb = sh.nb;
    const uint32_t m = na < 2u ? 1u : na + nb - 2u;
    // H[e]: the right chain, then the left one backwards without its ends
    auto H = [&](uint32_t e) { return e < na ? A.shared(e) : B.shared(m - e); };

    if (m < 3u) {
        if (tid == 0) {
            const uint32_t a = H(0);
            const int dx = m == 2u ? px(H(1)) - px(a) : 0, dy = m == 2u ? py(H(1)) - py(a) : 0;
            rec[0] = px(a), rec[1] = py(a), rec[2] = dx, rec[3] = dy;
            rec[4] = 0, rec[5] = dx * dx + dy * dy, rec[6] = 0, rec[7] = (int32_t)m;
        }
        return;
    }

    // search
    Cand best{kNone, 1u, 0u, 0, 0};
    for (uint32_t e = tid; e < m; e += kThreads) {
        const uint32_t a = H(e), b = H(e + 1u == m ? 0u : e + 1u);
        const int ax = px(a), ay = py(a), dx = px(b) - ax, dy = py(b) - ay;
        Cand c{e, (uint32_t)(dx * dx + dy * dy), 0u, 0, 0};
        c.hi = (int32_t)c.nn;  // t of a is 0, t of b is nn
        int hgt = 0;
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t p = H(k);
            const int qx = px(p) - ax, qy = py(p) - ay;
            const int t = dx * qx + dy * qy, s = dx * qy - dy * qx;  // |.| <= 2^29
            c.lo = min(c.lo, t), c.hi = max(c.hi, t), hgt = max(hgt, s);
        }
        c.hgt = (uint32_t)hgt;
        if (beats(c, best)) best = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand c;
        c.e = __shfl_xor(best.e, o), c.nn = __shfl_xor(best.nn, o), c.hgt = __shfl_xor(best.hgt, o);
        c.lo = __shfl_xor(best.lo, o), c.hi = __shfl_xor(best.hi, o);
        if (beats(c, best)) best = c;
    }
    if ((tid & 63u) == 0) sh.wave[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            if (beats(sh.wave[w], best)) best = sh.wave[w];
        const uint32_t a = H(best.e), b = H(best.e + 1u == m ? 0u : best.e + 1u);
        rec[0] = px(a), rec[1] = py(a), rec[2] = px(b) - px(a), rec[3] = py(b) - py(a);
        rec[4] = best.lo, rec[5] = best.hi, rec[6] = (int32_t)best.hgt, rec[7] = (int32_t)m;
    }
}

}  // namespace

extern "C" int64_t ipp_polygons_obb_scratch_bytes(int32_t n_images, int64_t total_vertices) {
    if (n_images < 0 || n_images >= kMaxImages || total_vertices < 0 || total_vertices > (1ll << 40)) return IPP_E_ARG;
    return chain_bytes(total_vertices);
}

extern "C" int ipp_polygons_obb(const int32_t* verts, const int64_t* offsets, const int32_t* hdr, int32_t n_images,
                                int64_t total_vertices, int32_t bg_w, int32_t bg_h, uint8_t* scratch, int32_t* obb,
                                void* stream) {
    if (!verts || !offsets || !hdr || !scratch || !obb) return IPP_E_ARG;
    if (n_images < 0 || n_images >= kMaxImages || total_vertices < 0 || total_vertices > (1ll << 40)) return IPP_E_ARG;
    if (bg_w < 1 || bg_w > kMaxCoord || bg_h < 1 || bg_h > kMaxCoord) return IPP_E_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15u) != 0) return IPP_E_ARG;
    if (((reinterpret_cast<uintptr_t>(verts) | reinterpret_cast<uintptr_t>(hdr) | reinterpret_cast<uintptr_t>(obb)) &
         3u) != 0 ||
        (reinterpret_cast<uintptr_t>(offsets) & 7u) != 0)
        return IPP_E_ARG;
    if (n_images == 0) return IPP_OK;
    hipLaunchKernelGGL(k_obb_rings, dim3((uint32_t)n_images), dim3(kThreads), 0, (hipStream_t)stream, verts, offsets,
                       hdr, reinterpret_cast<uint32_t*>(scratch), total_vertices, obb);
    IPP_CHECK_LAUNCH();
    return IPP_OK;
}
