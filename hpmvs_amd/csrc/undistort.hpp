// undistort.hpp -- VisualSFM one-parameter radial undistortion of a view's level 0 (reference Image::undistort,
// src/hpmvs/Image.cpp:68-146), written once for the device kernel (kernel_undistort.hip) and for the host
// restatement the tests compile with g++ (tests/undistort_host.cpp).
//
// Per output pixel the reference solves m (1 + k1 |m|^2) = p for the source point m in normalised coordinates with
// Cardano's formula: in float64 real arithmetic for k1 > 0, in std::complex<double> for k1 < 0.  The complex
// operations are restated here as the structures the reference's toolchain executes (libstdc++ <complex> of
// -std=c++11 on glibc, libgcc), not as textbook formulas:
//   sqrt(complex)         -> glibc csqrt; the argument is always real here (imaginary part +0)
//   pow(complex, double)  -> libstdc++: pow(real) for a positive real base, else polar(exp(y re(log z)), y im(log z))
//   log(complex)          -> glibc clog (log1p of x^2 + y^2 - 1 near |z| = 1, hypot + log elsewhere)
//   double / complex      -> libgcc __divdc3 (scaled Smith division)
//   complex * complex     -> the C99 product (ac - bd, ad + bc)
// sqrt and / are IEEE-exact on both sides; log, log1p, hypot, atan2, exp, sin, cos and pow are the platform's own
// (glibc on the host, the device library on the GPU).  NaN-recovery tails of __divdc3 / __muldc3 (both parts NaN) are
// not restated: they only act on inputs that already carry inf or NaN, and such a map is never sampled.
// Build with -ffp-contract=off: every product and sum below is a separately rounded operation in the reference.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define HPMVS_UD_FN __host__ __device__ inline
#define HPMVS_UD_UNROLL _Pragma("unroll")
#else
#define HPMVS_UD_FN inline
#define HPMVS_UD_UNROLL
#endif

namespace hpmvs {
namespace ud {

struct cplx {
    double re, im;
};

HPMVS_UD_FN bool is_nan(double v) { return v != v; }
HPMVS_UD_FN bool is_inf(double v) { return v == INFINITY || v == -INFINITY; }

// glibc csqrt for x + 0i
HPMVS_UD_FN cplx csqrt_real(double x) {
    if (is_nan(x)) return {NAN, NAN};
    if (is_inf(x)) return x < 0 ? cplx{0.0, INFINITY} : cplx{x, 0.0};
    if (x < 0) return {0.0, sqrt(-x)};
    return {fabs(sqrt(x)), 0.0};
}

// glibc __x2y2m1: x^2 + y^2 - 1 from the exact products, summed in order of magnitude (qsort is a stable merge sort
// there; an unrolled stable bubble sort keeps the five values in registers)
HPMVS_UD_FN void sort_abs(double* v, int from) {
HPMVS_UD_UNROLL
    for (int pass = 0; pass < 4; pass++)
HPMVS_UD_UNROLL
        for (int j = 0; j < 4; j++)
            if (j >= from && j < 4 - pass && fabs(v[j]) > fabs(v[j + 1])) {
                const double t = v[j];
                v[j] = v[j + 1];
                v[j + 1] = t;
            }
}
HPMVS_UD_FN double x2y2m1(double x, double y) {
    double v[5];
    v[1] = x * x;
    v[0] = fma(x, x, -v[1]);  // Dekker's split in glibc; both give the exact low part
    v[3] = y * y;
    v[2] = fma(y, y, -v[3]);
    v[4] = -1.0;
    sort_abs(v, 0);
HPMVS_UD_UNROLL
    for (int i = 0; i <= 3; i++) {
        const double a = v[i + 1], b = v[i];
        const double hi = a + b;
        v[i] = (a - hi) + b;
        v[i + 1] = hi;
        sort_abs(v, i + 1);
    }
    return v[4] + v[3] + v[2] + v[1] + v[0];
}

// glibc clog
HPMVS_UD_FN cplx clog_(cplx z) {
    if (z.re == 0 && z.im == 0) {
        const double im = 1.0 / z.re < 0 ? M_PI : 0.0;  // signbit of the zero real part
        return {-1.0 / fabs(z.re), copysign(im, z.im)};
    }
    if (is_nan(z.re) || is_nan(z.im)) return {(is_inf(z.re) || is_inf(z.im)) ? INFINITY : NAN, NAN};
    double absx = fabs(z.re), absy = fabs(z.im);
    int scale = 0;
    if (absx < absy) {
        const double t = absx;
        absx = absy;
        absy = t;
    }
    if (absx > DBL_MAX / 2) {
        scale = -1;
        absx = scalbn(absx, scale);
        absy = (absy >= DBL_MIN * 2 ? scalbn(absy, scale) : 0);
    } else if (absx < DBL_MIN && absy < DBL_MIN) {
        scale = DBL_MANT_DIG;
        absx = scalbn(absx, scale);
        absy = scalbn(absy, scale);
    }
    double re;
    if (absx == 1 && scale == 0) {
        re = log1p(absy * absy) / 2;
    } else if (absx > 1 && absx < 2 && absy < 1 && scale == 0) {
        double d2m1 = (absx - 1) * (absx + 1);
        if (absy >= DBL_EPSILON) d2m1 += absy * absy;
        re = log1p(d2m1) / 2;
    } else if (absx < 1 && absx >= 0.5 && absy < DBL_EPSILON / 2 && scale == 0) {
        const double d2m1 = (absx - 1) * (absx + 1);
        re = log1p(d2m1) / 2;
    } else if (absx < 1 && absx >= 0.5 && scale == 0 && absx * absx + absy * absy >= 0.5) {
        re = log1p(x2y2m1(absx, absy)) / 2;
    } else {
        const double d = hypot(absx, absy);
        re = log(d) - scale * M_LN2;
    }
    return {re, atan2(z.im, z.re)};
}

// libstdc++ pow(const complex<double>&, const double&) with C99 complex support
HPMVS_UD_FN cplx cpow_(cplx z, double y) {
    if (z.im == 0.0 && z.re > 0.0) return {pow(z.re, y), 0.0};
    const cplx t = clog_(z);
    const double rho = exp(y * t.re), theta = y * t.im;
    return {rho * cos(theta), rho * sin(theta)};  // std::polar
}

// libgcc __divdc3: (a + ib) / (c + id)
HPMVS_UD_FN cplx divdc3(double a, double b, double c, double d) {
    const double RBIG = DBL_MAX / 2, RMIN = DBL_MIN, RMIN2 = DBL_EPSILON, RMINSCAL = 1.0 / DBL_EPSILON,
                 RMAX2 = RBIG * RMIN2;
    double ratio, denom, x, y;
    if (fabs(c) < fabs(d)) {
        if (fabs(d) >= RBIG) { a = a / 2; b = b / 2; c = c / 2; d = d / 2; }
        if (fabs(d) < RMIN2) {
            a = a * RMINSCAL; b = b * RMINSCAL; c = c * RMINSCAL; d = d * RMINSCAL;
        } else if (((fabs(a) < RMIN) && (fabs(b) < RMAX2) && (fabs(d) < RMAX2)) ||
                   ((fabs(b) < RMIN) && (fabs(a) < RMAX2) && (fabs(d) < RMAX2))) {
            a = a * RMINSCAL; b = b * RMINSCAL; c = c * RMINSCAL; d = d * RMINSCAL;
        }
        ratio = c / d;
        denom = (c * ratio) + d;
        if (fabs(ratio) > RMIN) {
            x = ((a * ratio) + b) / denom;
            y = ((b * ratio) - a) / denom;
        } else {
            x = ((c * (a / d)) + b) / denom;
            y = ((c * (b / d)) - a) / denom;
        }
    } else {
        if (fabs(c) >= RBIG) { a = a / 2; b = b / 2; c = c / 2; d = d / 2; }
        if (fabs(c) < RMIN2) {
            a = a * RMINSCAL; b = b * RMINSCAL; c = c * RMINSCAL; d = d * RMINSCAL;
        } else if (((fabs(a) < RMIN) && (fabs(b) < RMAX2) && (fabs(c) < RMAX2)) ||
                   ((fabs(b) < RMIN) && (fabs(a) < RMAX2) && (fabs(c) < RMAX2))) {
            a = a * RMINSCAL; b = b * RMINSCAL; c = c * RMINSCAL; d = d * RMINSCAL;
        }
        ratio = d / c;
        denom = (d * ratio) + c;
        if (fabs(ratio) > RMIN) {
            x = ((b * ratio) + a) / denom;
            y = (b - (a * ratio)) / denom;
        } else {
            x = (a + (d * (b / c))) / denom;
            y = (b - (d * (a / c))) / denom;
        }
    }
    return {x, y};
}

// The source point output pixel (ix, iy) samples, in level-0 pixel coordinates (float, NaN possible), and whether the
// reference writes that pixel at all.  f and k1 are the reference's float members Image::f_ / k1_.
HPMVS_UD_FN bool source_point(int ix, int iy, int width, int height, float f, float k1, float* sx, float* sy) {
    float y = (float)(iy - height / 2.0);
    float x = (float)(ix - width / 2.0);
    x /= f;
    y /= f;
    if (y == 0) y = 1e-3;
    float mx, my;
    if (k1 == 0) {
        mx = x;
        my = y;
    } else {
        const double t2 = y * y;
        const double t3 = t2 * t2 * t2;
        const double t4 = x * x;
        const double t7 = k1 * (t2 + t4);
        if (k1 > 0) {
            const double t8 = 1.0 / t7;
            const double t10 = t3 / (t7 * t7);
            const double t14 = sqrt(t10 * (0.25 + t8 / 27.0));
            const double t15 = t2 * t8 * y * 0.5;
            const double t17 = pow(t14 + t15, 1.0 / 3.0);
            const double t18 = t17 - t2 * t8 / (t17 * 3.0);
            mx = t18 * x / y;
            my = t18;
        } else {
            const double t9 = t3 / (t7 * t7 * 4.0);
            const double t11 = t3 / (t7 * t7 * t7 * 27.0);
            const cplx t13 = csqrt_real(t9 + t11);
            const double t14 = t2 / t7;
            const double t15 = t14 * y * 0.5;
            const cplx t17 = cpow_(cplx{t13.re + t15, t13.im}, 1.0 / 3.0);
            const cplx q3 = divdc3(t14, 0.0, t17.re * 3.0, t17.im * 3.0);
            const cplx s = {t17.re + q3.re, t17.im + q3.im};
            const double r3 = sqrt(3.0);
            const cplx t18 = {s.re * 0.0 - s.im * r3, s.re * r3 + s.im * 0.0};
            const cplx q6 = divdc3(t14, 0.0, t17.re * 6.0, t17.im * 6.0);
            const double t19 = (t17.re + t18.re) * -0.5 + q6.re;
            mx = t19 * x / y;
            my = t19;
        }
    }
    x = mx * f + width / 2.0f;
    y = my * f + height / 2.0f;
    *sx = x;
    *sy = y;
    return x > 1 && x < width - 1 && y > 1 && y < height - 1;
}

// CImg _linear_atXY (thirdLibs/cimg/CImg.h:12218-12235) on channel c of interleaved u8 RGB, truncated back to u8 as
// `images_[0] = undistorted` does
HPMVS_UD_FN uint8_t sample(const uint8_t* src, int width, int height, float fx, float fy, int c) {
    const float nfx = fx < 0 ? 0 : (fx > width - 1 ? width - 1 : fx), nfy = fy < 0 ? 0 : (fy > height - 1 ? height - 1 : fy);
    const unsigned int x = (unsigned int)nfx, y = (unsigned int)nfy;
    const float dx = nfx - x, dy = nfy - y;
    const unsigned int nx = dx > 0 ? x + 1 : x, ny = dy > 0 ? y + 1 : y;
    const size_t w = (size_t)width;
    const float Icc = src[3 * (y * w + x) + c], Inc = src[3 * (y * w + nx) + c];
    const float Icn = src[3 * (ny * w + x) + c], Inn = src[3 * (ny * w + nx) + c];
    return (uint8_t)(Icc + dx * (Inc - Icc + dy * (Icc + Inn - Icn - Inc)) + dy * (Icn - Icc));
}

}  // namespace ud
}  // namespace hpmvs
