// ipp_resample_plan.h — the one host statement of Pillow Resample.c's
// precompute_coeffs + normalize_coeffs_8bpc (PRECISION_BITS = 22): the five
// filter functions with their supports, and per axis the scale, the support,
// each output's bounds and its normalised, quantised taps.  Host only
// (ipp_host.cpp, ipp_plan.cpp); the device statement is ipp_taps.hip.
//
// Every operation is in Resample.c's order, in double with the same libm
// sin(): plain mul/add, so the including files must not be built with
// floating-point contraction (x86-64 baseline g++, no FMA: Makefile HOSTFLAGS).
#pragma once
#include <math.h>
#include <stdint.h>

#include "ipp.h"

namespace resample_plan {

inline double box_filter(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }

inline double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

inline double hamming_filter(double x) {
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * M_PI;
    return sin(x) / x * (0.54f + 0.46f * cos(x));  // float literals, widened: as in Resample.c
}

inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

inline double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

inline double lanczos_filter(double x) {
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}

struct Filter {
    double (*f)(double);
    double support;
};
// indexed by IPP_RESAMPLE_*
inline const Filter kFilters[5] = {
    {box_filter, 0.5}, {bilinear_filter, 1.0}, {hamming_filter, 1.0}, {bicubic_filter, 2.0}, {lanczos_filter, 3.0}};
static_assert(IPP_RESAMPLE_BOX == 0 && IPP_RESAMPLE_LANCZOS == 4, "kFilters' order");

// One axis: in_size inputs, the box [in0, in1) of them resampled to out_size
// outputs (filter 0..4, in_size > 0, out_size > 0: the callers check).
struct Axis {
    const Filter& flt;
    int in_size;
    float fin0;  // Resample.c takes float box[4]
    double scale, support, ss;
    int ksize;

    Axis(int filter, int in_size_, double in0, double in1, int out_size) : flt(kFilters[filter]), in_size(in_size_) {
        fin0 = (float)in0;
        const float fin1 = (float)in1;
        scale = (double)(fin1 - fin0) / out_size;
        const double filterscale = scale < 1.0 ? 1.0 : scale;
        support = flt.support * filterscale;
        ss = 1.0 / filterscale;
        ksize = (int)ceil(support) * 2 + 1;
    }

    double center(int xx) const { return fin0 + (xx + 0.5) * scale; }

    // output xx reads inputs [xmin, xmin + cnt)
    void bounds(int xx, int& xmin, int& cnt) const {
        const double c = center(xx);
        xmin = (int)(c - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(c + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        cnt = xmax - xmin;
    }

    // bounds(xx) and the output's ksize quantised taps kq (zero past cnt);
    // k: ksize doubles of scratch
    void taps(int xx, double* k, int32_t* kq, int& xmin, int& cnt) const {
        bounds(xx, xmin, cnt);
        const double c = center(xx);
        double ww = 0.0;
        for (int x = 0; x < cnt; ++x) {
            const double w = flt.f((x + xmin - c + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < cnt; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (int x = 0; x < ksize; ++x) {
            const double v = x < cnt ? k[x] : 0.0;
            kq[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << 22)) : (int32_t)(0.5 + v * (1 << 22));
        }
    }
};

}  // namespace resample_plan
