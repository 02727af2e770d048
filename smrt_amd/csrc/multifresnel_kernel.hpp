// Multi-Fresnel thermal emission solver (the reference's smrt/rtsolver/multifresnel_thermalemission.py and
// multifresnel/multifresnel.py; Hebert et al. 2015, annex of Zeiger et al. 2024): the per-item arithmetic of its two kernels.
//
//   multifresnel_layer_item  one (pair, layer slot): effective permittivity, ks, ka (layer_em) ONCE per pair whatever the
//                            number of angles; slot n_layers of a pair on a Flat substrate is the substrate (1e10 m thick).
//                            Writes the staging rows [quantity][slot][pair] and the optional layer_out.
//   multifresnel_chain_item  one (pair, sensor angle), both polarisations (they share the refracted cosine and the
//                            attenuation): the running product of one 2 x 3 affine matrix per layer, left to right, in
//                            registers.  The trip count is the pair's own; no LDS, no cross-lane operation: the same source
//                            is compiled by g++ (-DSMRT_HOST_EMU) for the CPU tests.
//
// No Planck function: T is the physical temperature, as in the reference.
#pragma once
#include "dort_physics.hpp"

namespace smrt {

// staging rows, each [Lmax + 1][n_pairs]: permittivity, its square root, k0 x thickness (< 0: slot unused -1, invalid -2), T
enum { MF_EPS_RE = 0, MF_EPS_IM, MF_N_RE, MF_N_IM, MF_KD, MF_T, MF_ROWS };
constexpr int ST_NONFINITE = 8;              // smrt_dort.h: SMRT_ERR_NONFINITE
constexpr double kMfSubstrateDepth = 1e10;   // metres: the substrate as one more layer

struct MfBatch {
    int S, Lmax, F, n_theta;
    int emmodel, micro, sub_kind, steepest;     // steepest: index of the largest sensor cosine (the first of equals)
    double prune;                               // optical depth every angle starts with; +infinity: no pruning
    long long n_pairs;
    const long long* pair_map;                  // null: row i is pair i of the flattened f * S + s list
    const int* n_layers;
    const double *thickness, *frac_volume, *temperature, *p1, *p2, *frequency, *mu, *liquid_water;
    const int* layer_kind;
    const double *sub_p1, *sub_p2, *sub_T;      // [F][S], [F][S], [S]
    double* stage;                              // [MF_ROWS][Lmax + 1][n_pairs]
    double* out;                                // [n_pairs][n_theta][2] (V, H)
    int* status;                                // [n_pairs][n_theta]
    int* layers_used;                           // [n_pairs]
    double* tau_snowpack;                       // [n_pairs]
    double* layer_out;                          // [n_pairs][Lmax][5]
};

SMRT_DEV long long mf_global_pair(const MfBatch& b, long long i) { return b.pair_map ? b.pair_map[i] : i; }
SMRT_DEV double& mf_stage(const MfBatch& b, int row, int l, long long i) {
    return b.stage[((long long)row * (b.Lmax + 1) + l) * b.n_pairs + i];
}

// ---- kernel (a): one (pair, layer slot), slot in [0, Lmax] -----------------------------------------------------------------
SMRT_DEV void multifresnel_layer_item(const MfBatch& b, long long i, int l) {
    const long long gp = mf_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const double frequency = b.frequency[gp / b.S];
    const int L = b.n_layers[s];
    const double k0 = 2.0 * kPi * frequency / kCSpeed;
    double* lo = l < b.Lmax ? b.layer_out + (i * b.Lmax + l) * 5 : nullptr;
    cplx ee = cmk(1.0, 0.0);
    double kd = -1.0, T = 0.0;
    if (l < L) {
        const long long at = (long long)s * b.Lmax + l;
        const int kind = b.layer_kind ? b.layer_kind[at] : b.emmodel + 16 * b.micro;
        double ks, ka, pa, pb; int bad = 0;
        T = b.temperature[at];
        layer_em(kind & 15, kind >> 4, frequency, b.frac_volume[at], T, b.p1[at], b.p2 ? b.p2[at] : 0.0, &ee, &ks, &ka, &pa, &pb,
                 &bad, b.liquid_water ? b.liquid_water[at] : 0.0);
        kd = bad || !(b.thickness[at] > 0.0) ? -2.0 : k0 * b.thickness[at];
        lo[0] = ee.re; lo[1] = ee.im; lo[2] = ks; lo[3] = ka; lo[4] = 0.0;
    } else {
        if (lo) lo[0] = lo[1] = lo[2] = lo[3] = lo[4] = 0.0;
        if (l == L && b.sub_kind == SUB_FLAT) { ee = cmk(b.sub_p1[gp], b.sub_p2[gp]); T = b.sub_T[s]; kd = k0 * kMfSubstrateDepth; }
    }
    const cplx n = csqrt_(ee);
    mf_stage(b, MF_EPS_RE, l, i) = ee.re; mf_stage(b, MF_EPS_IM, l, i) = ee.im;
    mf_stage(b, MF_N_RE, l, i) = n.re; mf_stage(b, MF_N_IM, l, i) = n.im;
    mf_stage(b, MF_KD, l, i) = kd; mf_stage(b, MF_T, l, i) = T;
}

// ---- kernel (b): one (pair, sensor angle) ----------------------------------------------------------------------------------
// the 2 x 3 affine matrix of one polarisation (third row 0 0 1 implicit)
struct mf23 { double a00, a01, a02, a10, a11, a12; };

// interface with power reflectivity r on top of a layer of transmission t, 1 / t = it, at temperature T
SMRT_DEV mf23 mf_layer_matrix(double r, double t, double it, double T) {
    const double l13 = -(it - 1.0) * T, l23 = (1.0 - t) * T, q = 1.0 / (1.0 - r), c = 1.0 - 2.0 * r;
    mf23 m;
    m.a00 = it * q; m.a01 = -r * t * q; m.a02 = (l13 - r * l23) * q;
    m.a10 = r * it * q; m.a11 = c * t * q; m.a12 = (r * l13 + c * l23) * q;
    return m;
}
SMRT_DEV mf23 mf_mul(const mf23& a, const mf23& c) {
    mf23 m;
    m.a00 = a.a00 * c.a00 + a.a01 * c.a10; m.a01 = a.a00 * c.a01 + a.a01 * c.a11; m.a02 = a.a00 * c.a02 + a.a01 * c.a12 + a.a02;
    m.a10 = a.a10 * c.a00 + a.a11 * c.a10; m.a11 = a.a10 * c.a01 + a.a11 * c.a11; m.a12 = a.a10 * c.a02 + a.a11 * c.a12 + a.a12;
    return m;
}
SMRT_DEV double mf_emerging(const mf23& m) { return -m.a10 * m.a02 / m.a00 + m.a12; }

// -k_y of the transmitted wave (Maezawa & Miyauchi 2009 eq. 8) for the squared tangential wavenumber kz2
SMRT_DEV cplx mf_ky(cplx e, double kz2) { return cscale(csqrt_(cmk(e.re - kz2, e.im)), -1.0); }
// a / b by Smith's scaling with true divisions, as NumPy divides: a = -b gives -1 exactly, so that the reflectivity of a
// grazing angle (k_y of the incident wave 0) is exactly 1 and the result is non-finite as in the reference.  cdiv's
// a x conj(b) x (1 / |b|^2) rounds to 1 -+ 1 ulp for some b, and 1 / (1 - r) is then a finite, meaningless 1e16.
SMRT_DEV cplx mf_cdiv(cplx a, cplx b) {
    if (fabs(b.re) >= fabs(b.im)) {
        const double q = b.im / b.re, d = fma(b.im, q, b.re);
        return cmk(fma(a.im, q, a.re) / d, fma(-a.re, q, a.im) / d);
    }
    const double q = b.re / b.im, d = fma(b.re, q, b.im);
    return cmk(fma(a.re, q, a.im) / d, fma(a.im, q, -a.re) / d);
}
// optical depth of a layer, clipped to [0, limit] as numpy.clip does (a NaN passes through)
SMRT_DEV double mf_optical_depth(double n_im, double kd, double mu2, double limit) {
    double tau = 2.0 * n_im * kd / mu2;
    tau = tau < 0.0 ? 0.0 : tau;
    return tau > limit ? limit : tau;
}

SMRT_DEV void multifresnel_chain_item(const MfBatch& b, long long i, int t) {
    const long long gp = mf_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const int n_slots = b.n_layers[s] + (b.sub_kind == SUB_FLAT ? 1 : 0);
    double mu = b.mu[t], mu_s = b.mu[b.steepest];       // cosines in the medium above the current interface
    double rem = b.prune, rem_s = b.prune;              // optical depth this angle / the steepest angle has left
    double tau_snowpack = 0.0;
    int bad = !(mu >= 0.0 && mu <= 1.0), used = 0;
    cplx e1 = cmk(1.0, 0.0), n1 = cmk(1.0, 0.0);
    mf23 mv, mh;
    mv.a00 = mv.a11 = mh.a00 = mh.a11 = 1.0; mv.a01 = mv.a02 = mv.a10 = mv.a12 = mh.a01 = mh.a02 = mh.a10 = mh.a12 = 0.0;
    for (int l = 0; l < n_slots; ++l) {
        const cplx e2 = cmk(mf_stage(b, MF_EPS_RE, l, i), mf_stage(b, MF_EPS_IM, l, i));
        const cplx n2 = cmk(mf_stage(b, MF_N_RE, l, i), mf_stage(b, MF_N_IM, l, i));
        const double kd = mf_stage(b, MF_KD, l, i), T = mf_stage(b, MF_T, l, i);
        if (kd < 0.0) bad = 1;
        // rigorous Fresnel coefficients at the interface above the layer (core/fresnel.py:99-146) and the refracted cosine
        const double kz2 = n1.re * n1.re * (1.0 - mu * mu);
        const cplx kyi = mf_ky(e1, kz2), kyt = mf_ky(e2, kz2);
        const cplx rh = mf_cdiv(csub(kyi, kyt), cadd(cconj(kyi), kyt));
        const cplx rv = mf_cdiv(cmul(cconj(n1), csub(cmul(e2, kyi), cmul(e1, kyt))),
                             cmul(n1, cadd(cmul(e2, cconj(kyi)), cmul(cconj(e1), kyt))));
        const double mu2 = -kyt.re / n2.re;
        const double tau = mf_optical_depth(n2.im, kd, mu2, rem);
        const double tr = exp(-tau), itr = 1.0 / tr;
        const mf23 lv = mf_layer_matrix(cabs2(rv), tr, itr, T), lh = mf_layer_matrix(cabs2(rh), tr, itr, T);
        if (l == 0) { mv = lv; mh = lh; } else { mv = mf_mul(mv, lv); mh = mf_mul(mh, lh); }
        rem -= tau;
        // the steepest angle's own recurrence, carried by every lane of the pair: it decides the stop for all of them
        const double kz2_s = n1.re * n1.re * (1.0 - mu_s * mu_s);
        const double mu2_s = -mf_ky(e2, kz2_s).re / n2.re;
        const double tau_s = mf_optical_depth(n2.im, kd, mu2_s, rem_s);
        rem_s -= tau_s;
        tau_snowpack += tau_s;
        used = l + 1;
        if (rem_s < 0.0) break;
        mu = mu2; mu_s = mu2_s; e1 = e2; n1 = n2;
    }
    double tbv = mf_emerging(mv), tbh = mf_emerging(mh);
    int st = ST_OK;
    if (bad) { st = ST_INPUT; tbv = tbh = NAN; }
    else if (!(fabs(tbv) <= 1.79e308) || !(fabs(tbh) <= 1.79e308)) { st = ST_NONFINITE; tbv = tbh = NAN; }
    b.out[(i * b.n_theta + t) * 2] = tbv; b.out[(i * b.n_theta + t) * 2 + 1] = tbh;
    b.status[i * b.n_theta + t] = st;
    if (t == 0) { b.layers_used[i] = used; b.tau_snowpack[i] = tau_snowpack; }
}

}  // namespace smrt
