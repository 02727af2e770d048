// Complex helpers, layer electromagnetics (ice permittivity, mixing, IBA / DMRT coefficients, microstructure
// Fourier transforms), Planck functions and Fresnel coefficients.
// Part of the DORT device code (see dort_device.hpp for the overview and the reference map).
#pragma once
#include "spmd.hpp"
#include <math.h>
#include <string.h>
#include "dort_layout.hpp"

namespace smrt {

// ------------------------------------------------------------------------------------------------------------
// complex helpers
// ------------------------------------------------------------------------------------------------------------
struct cplx { double re, im; };
SMRT_DEV cplx cmk(double a, double b) { cplx z; z.re = a; z.im = b; return z; }
SMRT_DEV cplx cadd(cplx a, cplx b) { return cmk(a.re + b.re, a.im + b.im); }
SMRT_DEV cplx csub(cplx a, cplx b) { return cmk(a.re - b.re, a.im - b.im); }
SMRT_DEV cplx cmul(cplx a, cplx b) { return cmk(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re); }
SMRT_DEV cplx cscale(cplx a, double s) { return cmk(a.re * s, a.im * s); }
SMRT_DEV cplx cconj(cplx a) { return cmk(a.re, -a.im); }
SMRT_DEV double cabs2(cplx a) { return a.re * a.re + a.im * a.im; }
SMRT_DEV cplx cdiv(cplx a, cplx b) {
    double d = 1.0 / cabs2(b);
    return cmk((a.re * b.re + a.im * b.im) * d, (a.im * b.re - a.re * b.im) * d);
}
SMRT_DEV cplx csqrt_(cplx z) {  // principal branch
    if (z.re == 0.0 && z.im == 0.0) return cmk(0.0, 0.0);
    double m = sqrt(cabs2(z));
    double tt = sqrt(0.5 * (fabs(z.re) + m));
    if (z.re >= 0.0) return cmk(tt, z.im / (2.0 * tt));
    return cmk(fabs(z.im) / (2.0 * tt), z.im >= 0.0 ? tt : -tt);
}

// ------------------------------------------------------------------------------------------------------------
// layer electromagnetics
// ------------------------------------------------------------------------------------------------------------
SMRT_DEV cplx ice_permittivity(double frequency, double T) {  // Maetzler 2006, permittivity/ice.py:52-73
    double fg = frequency * 1e-9;
    double tc = T - kFreezing;
    double er = 3.1884 + 9.1e-4 * tc;
    double th = 300.0 / T - 1.0;
    double alpha = (0.00504 + 0.0062 * th) * exp(-22.1 * th);
    double eb = exp(335.0 / T);
    double betam = (0.0207 / T) * (eb / ((eb - 1.0) * (eb - 1.0))) + 1.16e-11 * fg * fg;
    double dbeta = exp(-9.963 + 0.0372 * tc);
    return cmk(er, alpha / fg + (betam + dbeta) * fg);
}

// Permittivity of liquid water, double Debye model of Maetzler & Wegmuller (1987) as smrt/permittivity/water.py:14-43
SMRT_DEV cplx water_permittivity(double frequency, double T) {
    const double fg = frequency * 1e-9;
    const double th = 1.0 - 300.0 / T;
    const double e0 = 77.66 - 103.3 * th;
    const double e1 = 0.0671 * e0;
    const double f1 = 20.2 + 146.4 * th + 316.0 * th * th;
    const double e2 = 3.52 + 7.52 * th;
    const double f2 = 39.8 * f1;
    const cplx a = cdiv(cmk(e1 - e2, 0.0), cmk(1.0, -fg / f2));
    const cplx b = cdiv(cmk(e0 - e1, 0.0), cmk(1.0, -fg / f1));
    return cadd(cmk(e2, 0.0), cadd(a, b));
}

SMRT_DEV double sinc_(double x) { return x == 0.0 ? 1.0 : sin(x) / x; }

// FT of the autocorrelation function at wavenumber k (k2 = k*k)
SMRT_DEV double ft_corr(int micro, double k2, double fv, double p1, double p2, double krho = 0.0) {
    if (micro == MS_EXP) {  // exponential.py:53-58
        double x = k2 * p1 * p1;
        double den = 1.0 + x;
        return fv * (1.0 - fv) * 8.0 * kPi * p1 * p1 * p1 / (den * den);
    }
    // The rational models at the COMPLEX wavenumber k^2 (1 + i krho) of the strong-contrast-expansion emmodels, whose phase
    // function evaluates the transform at 2 k0 sqrt(eps_eff) sin(Theta / 2) with eps_eff complex and keeps the real part
    // (sce_common.py:222-233, emmodel/common.py:107-117), X = k2 p1^2.  (The sphere models at a complex k r were built and
    // measured: inlined here their complex arithmetic cost the prep kernel of the headline pipeline 44 more spilled
    // registers and 0.25 ms per step on paths that pipeline never takes, as a function of its own still 21 -- not kept:
    // such layers go the dense route, rtsolver/dort.py; validate() refuses their codes.)
    if (__builtin_expect(micro == MS_EXPC, 0)) {   // exponential: Re 1 / (1 + X (1 + i krho))^2
        const double xr = k2 * p1 * p1, xi = xr * krho;
        const double a = 1.0 + xr, a2 = a * a, b2 = xi * xi, m = a2 + b2;
        return fv * (1.0 - fv) * 8.0 * kPi * p1 * p1 * p1 * (a2 - b2) / (m * m);
    }
    if (__builtin_expect(micro == MS_TSC, 0)) {   // Teubner-Strey (p2 = Y): Re 1 / ((1 + Y)^2 + 2 (1 - Y) Xc + Xc^2), Xc = X (1 + i krho)
        const double xr = k2 * p1 * p1, xi = xr * krho;
        const double y = p2;
        const double a = (1.0 + y) * (1.0 + y) + 2.0 * (1.0 - y) * xr + xr * xr - xi * xi;
        const double b = 2.0 * (1.0 - y) * xi + 2.0 * xr * xi;
        return fv * (1.0 - fv) * 8.0 * kPi * p1 * p1 * p1 * a / (a * a + b * b);
    }
    if (micro == MS_TS) {   // Teubner-Strey, teubner_strey.py:45-55: p1 = correlation length xi, p2 = Y = (2 pi xi / repeat distance)^2;
        // with a negative Y the same expression is the product of two Lorentzians of unified_teubner_strey.py:69-72
        // (smrt_amd/core/layer.py: device_microstructure_params)
        const double x = k2 * p1 * p1, y = p2;
        return fv * (1.0 - fv) * 8.0 * kPi * p1 * p1 * p1 / ((1.0 + y) * (1.0 + y) + 2.0 * (1.0 - y) * x + x * x);
    }
    // spheres of radius p1: sticky hard spheres (sticky_hard_spheres.py:63-130) and independent spheres
    // (independent_sphere.py:54-72) share the form factor of the sphere, vint = 3 (sin x - x cos x) / x^3 -- ONE pair of
    // sin / cos in the code of every kernel
    double f = fv, tau = p2, radius = p1;
    double x = sqrt(k2) * radius;
    double vd = 4.0 / 3.0 * kPi * radius * radius * radius;
    double tt = 0.0, fr = 0.0, c1 = 0.0, c2 = 0.0;
    if (micro == MS_SPHERE) {
        if (fabs(x) <= 1e-2) {   // series of vint (the closed form cancels like x^-2 there): 1 - x^2 / 10 + x^4 / 280
            const double x2 = x * x, v = 1.0 - x2 * (0.1 - x2 * (1.0 / 280.0));
            return f * (1.0 - f) * vd * v * v;
        }
    } else {
        if (__builtin_expect(tau < 0.0, 0)) tt = -tau;   // t given, not a stickiness (unified_sticky_hard_spheres.py:24-27)
        else if (isfinite(tau) && f > 0.0) {
            double disc = 36 * tau * tau * f * f - 72 * tau * f * f - 72 * tau * tau * f + 30 * f * f + 72 * tau * f +
                          36 * tau * tau - 12 * f;
            tt = (6 * tau * f - 6 * f - 6 * tau + sqrt(disc)) / (f * (f - 1.0));
        }
        fr = f / (1.0 - f);
        c1 = 1.0 - tt * f + 3.0 * fr;
        c2 = 3.0 - tt * (1.0 - f);
        if (fabs(x) <= 1e-3) {
            double den = fr * (c1 + c2) + 1.0;
            return f * vd / (den * den);
        }
    }
    const double sx = sin(x), cx = cos(x), sc = sx / x;
    double vint = 3.0 * (sc - cx) / (x * x);
    if (micro == MS_SPHERE) return f * (1.0 - f) * vd * vint * vint;
    double psi = sc / vint;
    double a = fr * (c1 + c2 * psi) + cx / vint;
    double b = fr * x + sx / vint;
    return f * vd / (a * a + b * b);
}

SMRT_DEV double shs_t(double f, double tau, int* bad) {  // sticky_hard_spheres.py:132-167
    if (isinf(tau)) return 0.0;
    double a = f / 12.0, b = -(tau + f / (1.0 - f)), c = (1.0 + 0.5 * f) / ((1.0 - f) * (1.0 - f));
    double disc = b * b - 4.0 * a * c;
    if (disc < 0.0) { *bad = 1; return 0.0; }
    double sq = sqrt(disc);
    double tt = (-b - sq) / (2.0 * a);
    if (tt * f * (1.0 - f) > 1.0 + 2.0 * f) tt = (-b + sq) / (2.0 * a);
    if (tt * f * (1.0 - f) > 1.0 + 2.0 * f) *bad = 1;
    return tt;
}

SMRT_DEV double planck_radiance(double frequency, double T) {  // core/lib.py:594-607
    if (!(T > 1e-10)) return 0.0;
    return (2.0 * kPlanck / (kCSpeed * kCSpeed)) * frequency * frequency * frequency /
           expm1((kPlanck / kBoltzmann) * frequency / T);
}
SMRT_DEV double planck_inverse(double frequency, double radiance) {  // core/lib.py:610-620
    if (!(radiance > 1e-40)) return 0.0;
    double x = (2.0 * kPlanck / (kCSpeed * kCSpeed)) * frequency * frequency * frequency / radiance;
    return (kPlanck / kBoltzmann) * frequency / log1p(x);
}

// One layer: effective permittivity, ks, ka and the parameters of its phase function.
// pa/pb/pc: IBA+exponential -> C(cosT) = pa / (1 + pb (1 - cosT))^2 ; IBA+SHS -> pa = iba_coeff, pb = kfac^2/2;
// DMRT -> pa = 1.5 ks.
// em / ms: the emmodel and the microstructure model of THIS layer (a snowpack may mix them, smrt/core/model.py:529-582).
// lw: liquid water of a wet layer (water volume / (ice + water volume)), 0 for dry snow.
SMRT_DEV void layer_em(int em, int ms, double frequency, double fv, double T, double p1, double p2, cplx* eps_eff,
                       double* ks, double* ka, double* pa, double* pb, int* bad, double lw = 0.0) {
    cplx es = ice_permittivity(frequency, T);
    if (T > kFreezing) *bad = 1;
    if (__builtin_expect(lw > 0.0, 0)) {
        // wet ice grains (wetice.py:12-45, Bohren & Huffman 1983 after Jin 1993 eq. 8-69): Maxwell Garnett mixing of ice
        // inclusions, volume fraction 1 - lw, in a water host (generic_mixing_formula.py:352-380); water after Maetzler &
        // Wegmuller 1987 (water.py:14-43), defined from the melting point up
        if (T < kFreezing || lw > 1.0) *bad = 1;
        const cplx ew = water_permittivity(frequency, T);
        const cplx cplus = cadd(es, cscale(ew, 2.0));
        const cplx cminus = cscale(csub(es, ew), 1.0 - lw);
        es = cmul(cdiv(cadd(cplus, cscale(cminus, 2.0)), csub(cplus, cminus)), ew);
    }
    double k0 = 2.0 * kPi * frequency / kCSpeed;
    if (em == EM_IBA || em == EM_IBA_INV) {
        // EM_IBA_INV: IBA's dense_snow_correction="auto" on a layer with more than half ice (iba.py:95-96,
        // core/layer.py:186-201): air inclusions (e1 = 1) in an ice background (e0 = ice); fv is then the AIR fraction,
        // which is what the caller passes for such a layer (smrt_dort.h)
        const cplx e0 = em == EM_IBA ? cmk(1.0, 0.0) : es, e1 = em == EM_IBA ? es : cmk(1.0, 0.0);
        const cplx de = csub(e1, e0);
        // Polder-van Santen, spheres: 2x^2 + bx - e1 e0 = 0 (generic_mixing_formula.py:117-145)
        cplx bq = csub(csub(e1, cscale(e0, 2.0)), cscale(de, 3.0 * fv));
        cplx disc = cadd(cmul(bq, bq), cscale(cmul(e1, e0), 8.0));
        cplx ee = cscale(csub(csqrt_(disc), bq), 0.25);
        if (ee.im < -1e-10) *bad = 1;
        *eps_eff = ee;
        // mean squared field ratio with depolarisation factors 1/3 (iba.py:152-162)
        cplx app = cadd(cscale(ee, 2.0 / 3.0), cscale(e0, 1.0 / 3.0));
        cplx den = cadd(app, cscale(de, 1.0 / 3.0));
        double y2 = cabs2(cdiv(app, den));
        double coeff = (1.0 / (4.0 * kPi)) * cabs2(de) * y2 * (k0 * k0) * (k0 * k0);
        cplx sq = csqrt_(ee);
        *ka = 2.0 * k0 * sq.im;  // iba.py:265
        // ks: Romberg on 65 samples of mu = 1 - j/32 (iba.py:176-226; scipy.integrate.romb), |sqrt(eps)| here
        double nabs2 = sqrt(cabs2(ee));  // |sqrt(eps)|^2 = |eps|
        double S[7];
        for (int i = 0; i < 7; ++i) S[i] = 0.0;
        double yend = 0.0;
        for (int j = 0; j <= 64; ++j) {
            double mu = 1.0 - j * 0.03125;
            double k2 = 4.0 * k0 * k0 * (0.5 * (1.0 - mu)) * nabs2;
            double y = coeff * ft_corr(ms, k2, fv, p1, p2) * (mu * mu + 1.0);
            if (j == 0 || j == 64) { yend += 0.5 * y; continue; }
            int tz = 0;
            while (((j >> tz) & 1) == 0) ++tz;
            for (int i = 6 - tz; i <= 6; ++i) S[i] += y;
        }
        double R[7];
        for (int i = 0; i < 7; ++i) R[i] = (double)(64 >> i) * 0.03125 * (yend + S[i]);
        double pw = 1.0;
        for (int j = 1; j <= 6; ++j) {
            pw *= 4.0;
            for (int i = 0; i <= 6 - j; ++i) R[i] = (pw * R[i + 1] - R[i]) / (pw - 1.0);
        }
        *ks = 0.25 * R[0];
        double kfac = 2.0 * k0 * sq.re;  // iba.py:233
        if (ms == MS_EXP) {
            *pa = coeff * fv * (1.0 - fv) * 8.0 * kPi * p1 * p1 * p1;
            *pb = 0.5 * kfac * kfac * p1 * p1;
        } else {
            *pa = coeff;
            *pb = 0.5 * kfac * kfac;
        }
    } else if (em == EM_NONSCAT) {
        // non-scattering medium (nonscattering.py): Polder-van Santen permittivity, absorption only
        cplx bq = csub(csub(es, cmk(2.0, 0.0)), cscale(csub(es, cmk(1.0, 0.0)), 3.0 * fv));
        cplx ee = cscale(csub(csqrt_(cadd(cmul(bq, bq), cscale(es, 8.0))), bq), 0.25);
        *eps_eff = ee;
        *ka = 2.0 * k0 * csqrt_(ee).im;
        *ks = 0.0; *pa = 0.0; *pb = 0.0;
    } else if (em == EM_QCACP) {
        // DMRT QCA-CP short range as in DMRT-ML (dmrt_qcacp_shortrange.py:63-125), dense_snow_correction="auto"
        double f = fv;
        cplx e0 = cmk(1.0, 0.0), e1 = es;
        if (f > 0.5) { f = 1.0 - f; e0 = es; e1 = cmk(1.0, 0.0); }
        int tb = 0;
        const double tt = shs_t(f, p2, &tb);
        if (tb) *bad = 1;
        const cplx de = csub(e1, e0);
        const cplx bq = csub(cscale(de, (1.0 - 4.0 * f) / 3.0), e0);
        const cplx cq = cscale(cmul(e0, de), -(1.0 - f) / 3.0);
        const cplx disc = csqrt_(csub(cmul(bq, bq), cscale(cq, 4.0)));
        cplx ee0 = cscale(csub(disc, bq), 0.5);
        if (ee0.re < 1.0) ee0 = cscale(cadd(disc, bq), -0.5);
        const double x = k0 * p1;  // 2 pi radius / lambda (vacuum wavelength)
        const double x3 = x * x * x;
        const double den = 1.0 + 2.0 * f - tt * f * (1.0 - f);
        const double omf4 = (1.0 - f) * (1.0 - f) * (1.0 - f) * (1.0 - f);
        const double shape = omf4 / (den * den);
        const cplx corr = cdiv(de, cadd(cmk(1.0, 0.0), cscale(cdiv(de, cscale(ee0, 3.0)), 1.0 - f)));
        const cplx fac = cadd(cmk(1.0, 0.0), cscale(cmul(cmul(cmk(0.0, 2.0 / 9.0 * x3), csqrt_(ee0)), corr), shape));
        const cplx ee = cadd(e0, cmul(csub(ee0, e0), fac));
        *eps_eff = ee;
        const double sqim = csqrt_(ee).im;
        const double albedo = 2.0 / 9.0 * x3 * f / (2.0 * sqim) * cabs2(corr) * shape;
        const double beta = 2.0 * k0 * sqim;
        *ks = albedo * beta;
        *ka = beta - albedo * beta;
        *pa = 1.5 * albedo * beta;
        *pb = 0.0;
    } else {
        // DMRT QCA short range (dmrt_qca_shortrange.py:65-112), dense_snow_correction="auto"
        double f = fv;
        cplx e0 = cmk(1.0, 0.0), e1 = es;
        if (f > 0.5) { f = 1.0 - f; e0 = es; e1 = cmk(1.0, 0.0); }
        int tb = 0;
        double tt = shs_t(f, p2, &tb);
        if (tb) *bad = 1;
        cplx y = cdiv(csub(e1, e0), cadd(e1, cscale(e0, 2.0)));
        cplx fy = cscale(y, f);
        double kk = k0 * csqrt_(e0).re;
        double kr3 = (kk * p1) * (kk * p1) * (kk * p1);
        double den = 1.0 + 2.0 * f - tt * f * (1.0 - f);
        double omf4 = (1.0 - f) * (1.0 - f) * (1.0 - f) * (1.0 - f);
        cplx one_m_fy = csub(cmk(1.0, 0.0), fy);
        // Eeff = e0 + 3 fy e0/(1-fy) * (1 + 2j/3 kr3 y (1-f)^4 / ((1-fy) den^2))
        cplx corr = cdiv(cscale(cmul(cmk(0.0, 2.0 / 3.0 * kr3 * omf4 / (den * den)), y), 1.0), one_m_fy);
        cplx fac = cadd(cmk(1.0, 0.0), corr);
        cplx ee = cadd(e0, cmul(cdiv(cmul(cscale(fy, 3.0), e0), one_m_fy), fac));
        *eps_eff = ee;
        double Ks = 2.0 / (9.0 * f) * kk * kr3 * (cabs2(csub(cdiv(ee, e0), cmk(1.0, 0.0))) * omf4 / (den * den));
        double beta = 2.0 * kk * csqrt_(ee).im;
        *ks = Ks;
        *ka = beta - Ks;
        *pa = 1.5 * Ks;
        *pb = 0.0;
    }
}

// Flat interface, Maezawa & Miyauchi 2009 "rigorous" Fresnel (core/fresnel.py:99-146): power R for V and H.
// field reflection coefficients and the cosine in medium 2
SMRT_DEV void fresnel_field(cplx e1, cplx e2, double mu1, cplx* rv, cplx* rh, double* mu2) {
    cplx n1 = csqrt_(e1);
    double kz2 = n1.re * n1.re * (1.0 - mu1 * mu1);
    cplx kyi = cscale(csqrt_(cmk(e1.re - kz2, e1.im)), -1.0);
    cplx kyt = cscale(csqrt_(cmk(e2.re - kz2, e2.im)), -1.0);
    *rh = cdiv(csub(kyi, kyt), cadd(cconj(kyi), kyt));
    cplx num = cmul(cconj(n1), csub(cmul(e2, kyi), cmul(e1, kyt)));
    cplx den = cmul(n1, cadd(cmul(e2, cconj(kyi)), cmul(cconj(e1), kyt)));
    *rv = cdiv(num, den);
    *mu2 = -kyt.re / csqrt_(e2).re;
}
SMRT_DEV void fresnel_RvRh(cplx e1, cplx e2, double mu1, double* Rv, double* Rh) {
    cplx rv, rh; double mu2;
    fresnel_field(e1, e2, mu1, &rv, &rh, &mu2);
    *Rv = cabs2(rv);
    *Rh = cabs2(rh);
}

// The rough soils of the passive solvers (smrt/substrate/soil_wegmuller.py, soil_qnh.py, rough_choudhury79.py): Fresnel's power
// reflection against the soil permittivity e2, seen from the last layer (e1, cosine mu1), then the model's adjustment of BOTH
// polarisations (QNH mixes them).  The parameters follow the [F][S] permittivities in the substrate arrays (smrt_dort.h): a0, a1
// from substrate_p1 and c0, c1 from substrate_p2 --
//   SUB_SOIL_WEGMULLER   a0 = roughness_rms;  R_h e^(-ksigma^sqrt(0.1 mu)), R_v = R_h mu^0.655 up to 60 degrees, R_h (0.635 - 0.0014
//                        (theta - 60)) beyond (the test is mu < cos(60 pi / 180), as the reference writes it)
//   SUB_SOIL_QNH         a0 = H, a1 = Q, c0 = Nv, c1 = Nh;  ((1 - Q) R_v + Q R_h) e^(-H mu^Nv) and likewise for H with Nh
//   SUB_ROUGH_CHOUDHURY  a0 = roughness_rms;  both times e^(-4 ksigma^2 mu^2); invalid where ksigma > 0.1
// ksigma = Re(2 pi f sqrt(e1 / c^2)) roughness_rms with c = 2.9979e8 as both models of the reference write it -- NOT kCSpeed: the
// 4e-6 between the two shows in a brightness temperature held to 1e-6 K.  Returns false where the model is out of its range.
constexpr double kSoilCSpeed = 2.9979e8;
constexpr double kChoudhuryKsigmaMax = 0.1;
SMRT_DEV double soil_ksigma(double frequency, cplx e1, double roughness_rms) {
    const double ic = 1.0 / kSoilCSpeed;
    return 2.0 * kPi * frequency * csqrt_(cscale(e1, ic * ic)).re * roughness_rms;
}
SMRT_DEV bool soil_in_range(int kind, double frequency, cplx e1, double a0) {
    return !(kind == SUB_ROUGH_CHOUDHURY && soil_ksigma(frequency, e1, a0) > kChoudhuryKsigmaMax);
}
// (not inlined: the transcendental functions of the models stay out of the register allocation of the kernels that call it once
// per (pair, stream), in a cold branch.  The strip and register-resident finish kernels call it from an instance of their own
// that is launched for soil batches only -- in the headline instance even the call cost the batch without a substrate scratch
// and 0.5 % of its time: dort_layout.hpp kSoilInstanceByDefault)
SMRT_DEV_NOINLINE bool soil_RvRh(int kind, double a0, double a1, double c0, double c1, double frequency, cplx e1, cplx e2, double mu1,
                        double* Rv, double* Rh) {
    double rv, rh;
    fresnel_RvRh(e1, e2, mu1, &rv, &rh);
    bool valid = true;
    if (kind == SUB_SOIL_QNH) {
        const double mv = ((1.0 - a1) * rv + a1 * rh) * exp(-a0 * pow(mu1, c0));
        rh = ((1.0 - a1) * rh + a1 * rv) * exp(-a0 * pow(mu1, c1));
        rv = mv;
    } else {
        const double ks = soil_ksigma(frequency, e1, a0);
        if (kind == SUB_SOIL_WEGMULLER) {
            rh *= exp(-pow(ks, sqrt(0.1 * mu1)));
            rv = (mu1 < cos(60.0 * kPi / 180.0)) ? rh * (0.635 - 0.0014 * (acos(mu1) * 180.0 / kPi - 60.0)) : rh * pow(mu1, 0.655);
        } else {
            valid = !(ks > kChoudhuryKsigmaMax);
            const double damping = exp(-4.0 * ks * ks * mu1 * mu1);
            rv *= damping; rh *= damping;
        }
    }
    *Rv = rv; *Rh = rh;
    return valid;
}

// R_v, R_h of the bottom boundary of a passive batch whose substrate is Flat or a rough soil, for the pair gp = f * S + si, seen
// from the last layer (el) under the cosine mu: what every passive kernel calls where it evaluates the substrate (DevBatch and
// SoBatch name the fields alike).  False where the soil model is out of its range (the kernels fail such a pair beforehand).
template <class Batch>
SMRT_DEV bool substrate_RvRh(const Batch& b, long long gp, int si, double frequency, cplx el, double mu, double* Rv, double* Rh) {
    const cplx es = cmk(b.sub_p1[gp], b.sub_p2[gp]);
    if (b.sub_kind == SUB_FLAT) { fresnel_RvRh(el, es, mu, Rv, Rh); return true; }
    const long long tail = (long long)b.F * b.S + 2 * si;
    return soil_RvRh(b.sub_kind, b.sub_p1[tail], b.sub_p1[tail + 1], b.sub_p2[tail], b.sub_p2[tail + 1], frequency, el, es, mu, Rv, Rh);
}
// A pair on a Choudhury substrate whose ksigma in the last layer (el) exceeds the model's range: status ST_INPUT
template <class Batch>
SMRT_DEV bool substrate_in_range(const Batch& b, int si, double frequency, cplx el) {
    return b.sub_kind != SUB_ROUGH_CHOUDHURY || soil_in_range(b.sub_kind, frequency, el, b.sub_p1[(long long)b.F * b.S + 2 * si]);
}

// DORT option process_coherent_layers (smrt/interface/coherent_flat.py:60-186): a layer thinner than 3/8 of a wavelength
// and its two flat interfaces collapsed into ONE interface between medium 1 (incidence, cosine mu1) and medium 2.
// Field reflection / transmission coefficients of the slab (Tsang I 5.2.10-14) and the cosine in medium 2.
struct SlabRT { cplx Rv, Rh, Tv, Th; double mu_t; };
SMRT_DEV SlabRT coherent_slab(double frequency, cplx e1, cplx e2, double mu1, cplx es, double thickness) {
    cplx r01v, r01h, r1tv, r1th; double mu_1, mu_t;
    fresnel_field(e1, es, mu1, &r01v, &r01h, &mu_1);
    fresnel_field(es, e2, mu_1 > 1e-4 ? mu_1 : 1e-4, &r1tv, &r1th, &mu_t);
    const cplx k1 = cscale(csqrt_(es), 2.0 * kPi * frequency / kCSpeed);
    const cplx ph = cscale(k1, mu_1 * thickness);                 // complex phase across the slab
    const double a1 = exp(-ph.im), a2 = a1 * a1;
    const cplx ex1 = cmk(a1 * cos(ph.re), a1 * sin(ph.re));       // exp(i phase)
    const cplx ex2 = cmk(a2 * cos(2.0 * ph.re), a2 * sin(2.0 * ph.re));
    const cplx one = cmk(1.0, 0.0);
    SlabRT o;
    const cplx dv = cadd(one, cmul(cmul(r01v, r1tv), ex2)), dh = cadd(one, cmul(cmul(r01h, r1th), ex2));
    o.Rv = cdiv(cadd(r01v, cmul(r1tv, ex2)), dv);
    o.Rh = cdiv(cadd(r01h, cmul(r1th, ex2)), dh);
    o.Tv = cdiv(cmul(cmul(cadd(one, r01v), cadd(one, r1tv)), ex1), dv);
    o.Th = cdiv(cmul(cmul(cadd(one, r01h), cadd(one, r1th)), ex1), dh);
    o.mu_t = mu_t;
    return o;
}
// Power reflection and transmission (V, H) of the interface between media 1 and 2, flat (slab_thickness == 0: rigorous
// Fresnel, T = 1 - R) or coherent (coherent_flat.py:76-147)
SMRT_DEV void interface_RT(double frequency, cplx e1, cplx e2, double mu1, cplx es, double slab_thickness,
                           double* Rv, double* Rh, double* Tv, double* Th) {
    if (!(slab_thickness > 0.0)) {
        fresnel_RvRh(e1, e2, mu1, Rv, Rh);
        *Tv = 1.0 - *Rv; *Th = 1.0 - *Rh;
        return;
    }
    const SlabRT q = coherent_slab(frequency, e1, e2, mu1, es, slab_thickness);
    const double nt = csqrt_(cdiv(e2, e1)).re;
    *Rv = cabs2(q.Rv); *Rh = cabs2(q.Rh);
    *Tv = cabs2(q.Tv) * q.mu_t / mu1 / nt;
    *Th = cabs2(q.Th) * q.mu_t / mu1 * nt;
}

}  // namespace smrt
