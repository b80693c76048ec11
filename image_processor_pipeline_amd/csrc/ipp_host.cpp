// ipp_host.cpp — host-side planning for the hot path (CPU, C ABI).
//
// These functions reproduce the HOST arithmetic of the libraries the
// reference calls, so the device kernels receive the exact integers Pillow
// would use:
//   * ipp_plan_resample: Pillow Resample.c precompute_coeffs +
//     normalize_coeffs_8bpc (ipp_resample_plan.h states them, once) for BOX,
//     BILINEAR, HAMMING, BICUBIC and LANCZOS — the taps of Image.resize behind
//     ipp_scene_feed_resize; ipp_plan_lanczos: its LANCZOS case, the taps
//     behind overlays.py:129.
//   * ipp_plan_mfma_tile: those LANCZOS taps as one MFMA tap tile of the
//     fused pipe, the only host packer of that format.
//   * ipp_plan_opaque_bbox: the getbbox() of rotations.py:99 for an opaque
//     source, solved per canvas row from the 16.16 affine map with exact
//     integer inequalities (no canvas is materialised).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ipp.h"
#include "ipp_pipe_layout.h"
#include "ipp_resample_plan.h"

using resample_plan::Axis;

namespace {

// floor(a / b) and ceil(a / b) for b != 0 (int64).
inline int64_t floordiv(int64_t a, int64_t b) {
    int64_t q = a / b, r = a % b;
    return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q;
}
inline int64_t ceildiv(int64_t a, int64_t b) { return -floordiv(-a, b); }

// X range where lo <= c + X*a <= hi (inclusive); returns false if empty.
inline bool solve_range(int64_t c, int64_t a, int64_t lo, int64_t hi, int64_t& xlo, int64_t& xhi) {
    if (a == 0) {
        if (c < lo || c > hi) return false;
        xlo = INT64_MIN / 4;
        xhi = INT64_MAX / 4;
        return true;
    }
    if (a > 0) {
        xlo = ceildiv(lo - c, a);
        xhi = floordiv(hi - c, a);
    } else {
        xlo = ceildiv(hi - c, a);
        xhi = floordiv(lo - c, a);
    }
    return xlo <= xhi;
}

}  // namespace

extern "C" int32_t ipp_plan_lanczos_ksize(double in0, double in1, int32_t out_size) {
    if (out_size <= 0) return IPP_E_ARG;
    return Axis(IPP_RESAMPLE_LANCZOS, 1, in0, in1, out_size).ksize;
}

extern "C" int64_t ipp_plan_resample(int32_t filter, int32_t in_size, double in0, double in1, int32_t out_size,
                                     int32_t* out, int64_t out_capacity) {
    if (filter < 0 || filter > 4 || in_size <= 0 || out_size <= 0) return IPP_E_ARG;
    const Axis ax(filter, in_size, in0, in1, out_size);
    const int64_t need = 2 * (int64_t)out_size + (int64_t)out_size * ax.ksize;
    if (out == nullptr) return -need;
    if (out_capacity < need) return IPP_E_ARG;
    int32_t* bounds = out;
    int32_t* kk = out + 2 * (int64_t)out_size;
    std::vector<double> k(ax.ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        int xmin, cnt;
        ax.taps(xx, k.data(), kk + (int64_t)xx * ax.ksize, xmin, cnt);
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = cnt;
    }
    return ax.ksize;
}

extern "C" int64_t ipp_plan_lanczos(int32_t in_size, double in0, double in1, int32_t out_size, int32_t* out,
                                    int64_t out_capacity) {
    return ipp_plan_resample(IPP_RESAMPLE_LANCZOS, in_size, in0, in1, out_size, out, out_capacity);
}

extern "C" int ipp_plan_opaque_bbox(int32_t in_w, int32_t in_h, const int32_t a[6], int32_t nw, int32_t nh,
                                    int32_t bbox[4]) {
    if (in_w <= 0 || in_h <= 0 || nw <= 0 || nh <= 0 || !a || !bbox) return IPP_E_ARG;
    int64_t x0 = INT64_MAX, x1 = -1, y0 = INT64_MAX, y1 = -1;
    const int64_t ux = (int64_t)in_w * 65536 - 1, uy = (int64_t)in_h * 65536 - 1;
    for (int64_t Y = 0; Y < nh; ++Y) {
        const int64_t cx = (int64_t)a[2] + Y * a[1];
        const int64_t cy = (int64_t)a[5] + Y * a[4];
        int64_t lo1, hi1, lo2, hi2;
        if (!solve_range(cx, a[0], 0, ux, lo1, hi1)) continue;
        if (!solve_range(cy, a[3], 0, uy, lo2, hi2)) continue;
        const int64_t lo = std::max<int64_t>(std::max(lo1, lo2), 0);
        const int64_t hi = std::min<int64_t>(std::min(hi1, hi2), nw - 1);
        if (lo > hi) continue;
        x0 = std::min(x0, lo);
        x1 = std::max(x1, hi);
        y0 = std::min(y0, Y);
        y1 = std::max(y1, Y);
    }
    if (x1 < 0) {
        bbox[0] = bbox[1] = bbox[2] = bbox[3] = -1;
    } else {
        bbox[0] = (int32_t)x0;
        bbox[1] = (int32_t)y0;
        bbox[2] = (int32_t)x1 + 1;
        bbox[3] = (int32_t)y1 + 1;
    }
    return IPP_OK;
}

extern "C" const char* ipp_version(void) { return "ipp 0.1.0 (gfx950)"; }

// The gather sampler of ipp_sampler.h make_sampler, once per image on the
// host (rotations.py:96 affine with symmetry.py:114-119's flip and the bbox
// crop of :99-101 folded in; 32-bit wrap-around as in the kernels).
extern "C" int ipp_gather_prepare(ipp_gather_desc* descs, int32_t n) {
    if (n < 0 || (n > 0 && !descs)) return IPP_E_ARG;
    for (int32_t i = 0; i < n; ++i) {
        ipp_gather_desc& g = descs[i];
        g.base_off = g.src_off + (int64_t)g.in_y0 * g.src_pitch + (int64_t)g.in_x0 * g.src_cn;
        const int64_t avail = (int64_t)(g.src_h - g.in_y0) * g.src_pitch - (int64_t)g.in_x0 * g.src_cn;
        g.lim = avail < 4 ? 0u : (uint32_t)(avail - 4);  // (avail = 3: a 1×1 window on the source's last pixel)
        const uint32_t sgx = (g.flip & 1) ? 0xFFFFFFFFu : 1u, sgy = (g.flip & 2) ? 0xFFFFFFFFu : 1u;
        const uint32_t sx0 = (uint32_t)(g.off_x + ((g.flip & 1) ? g.out_w - 1 : 0));
        const uint32_t sy0 = (uint32_t)(g.off_y + ((g.flip & 2) ? g.out_h - 1 : 0));
        g.b[0] = (int32_t)(sgx * (uint32_t)g.a0);
        g.b[1] = (int32_t)(sgy * (uint32_t)g.a1);
        g.b[2] = (int32_t)((uint32_t)g.a2 + sy0 * (uint32_t)g.a1 + sx0 * (uint32_t)g.a0);
        g.b[3] = (int32_t)(sgx * (uint32_t)g.a3);
        g.b[4] = (int32_t)(sgy * (uint32_t)g.a4);
        g.b[5] = (int32_t)((uint32_t)g.a5 + sy0 * (uint32_t)g.a4 + sx0 * (uint32_t)g.a3);
        g.prepared = 1;
    }
    return IPP_OK;
}

// Balanced signed bytes of a 22-bit tap: k = b0 + 256 b1 + 65536 b2, each
// b in [-128, 127] (the MFMA tile format, ipp_pipe_layout.h).
namespace {

inline void balanced_bytes(int32_t k, int8_t b[3]) {
    int32_t r = k;
    for (int p = 0; p < 3; ++p) {
        int32_t lo = ((r + 128) & 255) - 128;
        b[p] = (int8_t)lo;
        r = (r - lo) >> 8;
    }
}

}  // namespace

// The MFMA tile format of the fused pipe (hdr, bias, blocks; dense and compact
// tiles) is stated in ipp_pipe_layout.h; the functions below write it.
using namespace pipe_layout;

namespace {
inline int mfma_nk_bound(int32_t in_size, int32_t out_size, int32_t ksize) {
    const double scale = (double)in_size / (double)out_size;
    return (int)((16 + (int64_t)ceil(15.0 * scale) + 2 + ksize + 63) / 64);
}
}  // namespace

extern "C" int64_t ipp_plan_mfma_size(int32_t in_size, int32_t out_size, int32_t ksize) {
    if (in_size <= 0 || out_size <= 0 || ksize <= 0) return IPP_E_ARG;
    const int64_t T = tap_ntiles(out_size, 0) + 1;  // + 1: a phase may add a tile
    return tap_axis_words(T, mfma_nk_bound(in_size, out_size, ksize));
}

extern "C" int32_t ipp_plan_mfma_nk_bound(int32_t in_size, int32_t out_size, int32_t ksize) {
    if (in_size <= 0 || out_size <= 0 || ksize <= 0) return IPP_E_ARG;
    return mfma_nk_bound(in_size, out_size, ksize);
}

// One tile of an axis in the layout of the device tap planner (every tile
// with nkb K-step slots: tap_tile_block), from Pillow's taps computed here.
// The only host code that turns taps into {hdr, bias, blocks}.
extern "C" int ipp_plan_mfma_tile(const ipp_tap_axis* a, int32_t t, int32_t hdr[4], int32_t bias[16],
                                  uint8_t* blocks, int64_t blocks_cap) {
    if (!a || !hdr || !bias || !blocks || a->in_size <= 0 || a->out_size <= 0 || a->phase < 0 || a->phase > 15 ||
        t < 0 || t >= tap_ntiles(a->out_size, a->phase))
        return IPP_E_ARG;
    const int in = a->in_size, out = a->out_size, shift = a->shift;
    const int o0 = 16 * t - a->phase, o1 = std::min(o0 + 16, out), oa = std::max(o0, 0);
    const Axis ax(IPP_RESAMPLE_LANCZOS, in, 0.0, (double)in, out);
    const int ksize = a->identity ? 1 : ax.ksize;
    std::vector<double> kd(ksize);
    std::vector<int32_t> kq(16 * (size_t)ksize);
    int xs[16], cn[16];
    for (int o = oa; o < o1; ++o) {
        const int c = o - o0;
        if (a->identity) {
            xs[c] = o;
            cn[c] = 1;
            kq[(size_t)c * ksize] = 1 << 22;
        } else {
            ax.taps(o, kd.data(), kq.data() + (size_t)c * ksize, xs[c], cn[c]);
        }
        xs[c] -= shift;
    }
    if (xs[oa - o0] < 0) return IPP_E_RANGE;
    const int K0 = xs[oa - o0] & ~15;
    int end = K0;
    for (int o = oa; o < o1; ++o) end = std::max(end, xs[o - o0] + cn[o - o0]);
    const int nK = (end - K0 + 63) / 64;
    if (nK > a->nkb || (int64_t)nK * kKStepBytes > blocks_cap) return IPP_E_RANGE;
    // compact layout: each output's nonzero 16-column groups
    int g0[16], len[16], base[16], nb = 0;
    for (int col = 0; col < 16; ++col) {
        const int o = o0 + col;
        const bool valid = o >= oa && o < o1 && cn[col] > 0;
        g0[col] = valid ? (xs[col] - K0) >> 4 : 0;
        len[col] = valid ? ((xs[col] + cn[col] - 1 - K0) >> 4) - g0[col] + 1 : 0;
        base[col] = nb;
        nb += len[col];
    }
    const bool compact = a->compact && !a->identity && nK >= 2 && nb <= 64;
    hdr[0] = K0;
    hdr[1] = nK;
    hdr[2] = (int32_t)tap_tile_block(t, a->nkb);
    hdr[3] = compact ? 1 : 0;
    memset(blocks, 0, (size_t)nK * kKStepBytes);
    if (compact)
        for (int col = 0; col < 16; ++col) {
            const int32_t m = g0[col] | len[col] << 8 | base[col] << 16;
            memcpy(blocks + 4 * col, &m, 4);
        }
    for (int col = 0; col < 16; ++col) {
        const int o = o0 + col;
        if (o < oa || o >= o1) {
            bias[col] = 0;
            continue;
        }
        int64_t sum = 0;
        for (int q = 0; q < cn[col]; ++q) {
            const int32_t k = kq[(size_t)col * ksize + q];
            sum += k;
            int8_t b[3];
            balanced_bytes(k, b);
            const int rel = xs[col] + q - K0;
            if (compact) {
                const int i = base[col] + (rel >> 4) - g0[col], j = rel & 15;
                for (int p = 0; p < 3; ++p) blocks[(int64_t)tap_compact_block(p, i) * 16 + j] = (uint8_t)b[p];
            } else {
                const int s = rel / 64, kin = rel % 64;
                const int lane = 16 * (kin / 16) + col, j = kin % 16;
                for (int p = 0; p < 3; ++p) blocks[(int64_t)tap_dense_block(s, p, lane) * 16 + j] = (uint8_t)b[p];
            }
        }
        bias[col] = (int32_t)((1 << 21) + 128 * sum);
    }
    return IPP_OK;
}
