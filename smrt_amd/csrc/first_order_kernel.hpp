// Iterative first-order backscatter solver (the reference's smrt/rtsolver/iterative_first_order.py; Ulaby et al. 2014
// eqs. 11.62, 11.74, 11.75, refraction factor of Tsang et al. 2007 eqs. 22a/b): the per-item arithmetic of its two kernels.
//
//   first_order_layer_item  one (pair, layer): the layer electromagnetics (layer_em, or the caller's scalars for the
//                           host kinds), ONCE per pair whatever the number of incidence angles -- IBA's ks is a 65-point
//                           Romberg sum.  Writes the staging rows [quantity][layer][pair] that the second kernel reads
//                           with unit stride, and the optional layer_out.
//   first_order_angle_item  one (pair, incidence angle): the recursion from the surface down.  Carried state: the
//                           downward intensity I (2 x 2) and the cumulative upward transmission (diagonal); the four
//                           contributions are accumulated in registers.  No LDS, no cross-lane operation: the same
//                           source is compiled by g++ (-DSMRT_HOST_EMU) for the CPU tests.
//
// Everything is closed form: Fresnel coefficients, four samples of the phase matrix at azimuth pi and one exponential
// per layer.  Rough interfaces / substrates and emmodels without a device phase function arrive as numbers
// (include/smrt_dort.h: smrt_first_order_extras).
#pragma once
#include "dort_physics.hpp"

namespace smrt {

// staging rows, each [Lmax][n_pairs]
enum { FO_EPS_RE = 0, FO_EPS_IM, FO_KS, FO_KA, FO_PA, FO_PB, FO_KIND, FO_THICK, FO_FV, FO_P1, FO_P2, FO_ROWS };
// doubles per (pair, interface slot, angle) of the host-evaluated interfaces: specular reflection V, H; downward coherent
// transmission V, H; upward coherent transmission V, H; diffuse reflection at (mu, mu, pi): vv, vh, hv, hh
constexpr int kFoInterfaceDoubles = 10;
// doubles per (pair, layer, angle) of the optional carry: downward intensity in the layer V, H (it stays diagonal), cumulative
// upward transmission V, H, cosine of the incidence direction in the layer -- what second_order_kernel.hpp applies its terms to
constexpr int kFoCarryDoubles = 5;

struct FoBatch {
    int S, Lmax, F, n_theta;
    int emmodel, micro, sub_kind, n_slots;
    long long n_pairs;              // pairs of this launch (rows of every output)
    const long long* pair_map;      // null: row i is pair i of the flattened f * S + s list; else pair pair_map[i]
    const int* n_layers;
    const double *thickness, *frac_volume, *temperature, *p1, *p2, *frequency, *theta, *liquid_water;
    const int* layer_kind;
    const double *host_layer, *host_coeff;      // as smrt_batch: indexed by the global pair
    const double *sub_p1, *sub_p2;              // [F][S]
    const int* itf_slot;                        // [F * S][Lmax + 1] or null
    const double* itf_values;                   // [F * S][n_slots][n_theta][10]
    const double* host_phase;                   // [F * S][Lmax][n_theta][4][2][2] or null
    double* stage;                              // [FO_ROWS][Lmax][n_pairs]
    double* out;                                // [n_pairs][4][n_theta][2][2]
    int* status;                                // [n_pairs]
    double* layer_out;                          // [n_pairs][Lmax][5] or null
    double* layer_backscatter;                  // [n_pairs][Lmax + 1][n_theta][2][2] or null
    double* diag;                               // [n_pairs][2] or null
    double* carry;                              // [n_pairs][Lmax][n_theta][5] or null: a store only, the results do not depend on it
};

SMRT_DEV long long fo_global_pair(const FoBatch& b, long long i) { return b.pair_map ? b.pair_map[i] : i; }
SMRT_DEV double& fo_stage(const FoBatch& b, int row, int l, long long i) {
    return b.stage[((long long)row * b.Lmax + l) * b.n_pairs + i];
}

// ---- kernel (a): one (pair, layer) -------------------------------------------------------------------------------------
SMRT_DEV void first_order_layer_item(const FoBatch& b, long long i, int l) {
    const long long gp = fo_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const double frequency = b.frequency[gp / b.S];
    const int L = b.n_layers[s];
    double* lo = b.layer_out ? b.layer_out + (i * b.Lmax + l) * 5 : nullptr;
    if (l >= L) {
        fo_stage(b, FO_KIND, l, i) = -1.0;
        if (lo) lo[0] = lo[1] = lo[2] = lo[3] = lo[4] = 0.0;
        return;
    }
    const long long at = (long long)s * b.Lmax + l;
    const int kind = b.layer_kind ? b.layer_kind[at] : b.emmodel + 16 * b.micro;
    const int em = kind & 15, ms = kind >> 4;
    const double fv = b.frac_volume[at], p1 = b.p1[at], p2 = b.p2 ? b.p2[at] : 0.0;
    cplx ee; double ks, ka, pa = 0.0, pb = 0.0; int bad = 0;
    if (em == EM_HOST || em == EM_IBA_HOST || em == EM_RAYLEIGH_HOST) {   // scalars from the caller (smrt_batch.host_layer)
        if (b.host_layer) {
            const double* h = b.host_layer + (gp * b.Lmax + l) * 4;
            ks = h[0]; ka = h[1]; ee = cmk(h[2], h[3]);
            if (!(ka >= 0.0) || !(ee.re > 0.0)) bad = 1;
        } else { ks = ka = 0.0; ee = cmk(1.0, 0.0); bad = 1; }
        if (em == EM_RAYLEIGH_HOST) pa = 1.5 * ks;
        if (em == EM_IBA_HOST) {   // IBA's phase function with the caller's coefficient: pa / pb as layer_em leaves them
            const double coeff = b.host_coeff ? b.host_coeff[gp * b.Lmax + l] : -1.0;
            if (!(coeff >= 0.0) || ms >= MS_EXPC) bad = 1;
            const double kfac = 2.0 * (2.0 * kPi * frequency / kCSpeed) * csqrt_(ee).re;
            if (ms == MS_EXP) { pa = coeff * fv * (1.0 - fv) * 8.0 * kPi * p1 * p1 * p1; pb = 0.5 * kfac * kfac * p1 * p1; }
            else { pa = coeff; pb = 0.5 * kfac * kfac; }
        }
        if (em == EM_HOST && !b.host_phase && ks != 0.0) bad = 1;
    } else {
        layer_em(em, ms, frequency, fv, b.temperature[at], p1, p2, &ee, &ks, &ka, &pa, &pb, &bad,
                 b.liquid_water ? b.liquid_water[at] : 0.0);
    }
    if (!(ks >= 0.0) || !(b.thickness[at] > 0.0)) bad = 1;
    // the phase function the second kernel evaluates: IBA's (EM_IBA), Rayleigh's (EM_DMRT), none, or the caller's samples
    const int phase = (em == EM_IBA || em == EM_IBA_INV || em == EM_IBA_HOST) ? EM_IBA
                      : em == EM_NONSCAT ? EM_NONSCAT : em == EM_HOST ? EM_HOST : EM_DMRT;
    fo_stage(b, FO_EPS_RE, l, i) = ee.re; fo_stage(b, FO_EPS_IM, l, i) = ee.im;
    fo_stage(b, FO_KS, l, i) = ks; fo_stage(b, FO_KA, l, i) = ka;
    fo_stage(b, FO_PA, l, i) = pa; fo_stage(b, FO_PB, l, i) = pb;
    fo_stage(b, FO_KIND, l, i) = bad ? -2.0 : (double)(phase + 16 * ms);
    fo_stage(b, FO_THICK, l, i) = b.thickness[at];
    fo_stage(b, FO_FV, l, i) = fv; fo_stage(b, FO_P1, l, i) = p1; fo_stage(b, FO_P2, l, i) = p2;
    if (lo) { lo[0] = ee.re; lo[1] = ee.im; lo[2] = ks; lo[3] = ka; lo[4] = 0.0; }
}

// ---- kernel (b): one (pair, incidence angle) ---------------------------------------------------------------------------
struct m22 { double vv, vh, hv, hh; };   // [scattered polarisation][incident polarisation]
SMRT_DEV m22 m22_zero() { m22 m; m.vv = m.vh = m.hv = m.hh = 0.0; return m; }
SMRT_DEV m22 m22_mul(const m22& a, const m22& c) {
    m22 m;
    m.vv = a.vv * c.vv + a.vh * c.hv; m.vh = a.vv * c.vh + a.vh * c.hh;
    m.hv = a.hv * c.vv + a.hh * c.hv; m.hh = a.hv * c.vh + a.hh * c.hh;
    return m;
}
SMRT_DEV m22 m22_add(const m22& a, const m22& c) { m22 m; m.vv = a.vv + c.vv; m.vh = a.vh + c.vh; m.hv = a.hv + c.hv; m.hh = a.hh + c.hh; return m; }
SMRT_DEV m22 m22_scale(const m22& a, double s) { m22 m; m.vv = a.vv * s; m.vh = a.vh * s; m.hv = a.hv * s; m.hh = a.hh * s; return m; }
// diag(dv, dh) a   and   a diag(dv, dh)
SMRT_DEV m22 m22_left(double dv, double dh, const m22& a) { m22 m; m.vv = dv * a.vv; m.vh = dv * a.vh; m.hv = dh * a.hv; m.hh = dh * a.hh; return m; }
SMRT_DEV m22 m22_right(const m22& a, double dv, double dh) { m22 m; m.vv = a.vv * dv; m.vh = a.vh * dh; m.hv = a.hv * dv; m.hh = a.hh * dh; return m; }

// what the recursion needs of one layer
struct FoLayerPhase { int phase, ms; double pa, pb, fv, p1, p2; };

// Phase matrix (V, H) / 4 pi at azimuth pi between the cosines mu_s (scattered) and mu_i (incident): Rayleigh geometry of
// the scattering amplitudes times the emmodel's angular function (emmodel/common.py: Tsang's convention)
SMRT_DEV m22 fo_phase(const FoLayerPhase& q, double mu_s, double mu_i) {
    const double cphi = -1.0, sphi = 1.2246467991473532e-16;   // cos(pi), and sin(pi) as the reference's doubles have it
    const double ss = sqrt(1.0 - mu_s * mu_s), si = sqrt(1.0 - mu_i * mu_i);
    const double fvv = cphi * mu_s * mu_i + ss * si, fvh = sphi * mu_s, fhv = -sphi * mu_i, fhh = cphi;
    double C;
    if (q.phase == EM_IBA) {
        double ct = mu_s * mu_i + ss * si * cphi;
        ct = ct > 1.0 ? 1.0 : (ct < -1.0 ? -1.0 : ct);
        if (q.ms == MS_EXP) { const double dp = 1.0 + q.pb * (1.0 - ct); C = q.pa / (dp * dp); }
        else C = q.pa * ft_corr(q.ms, q.pb * (1.0 - ct), q.fv, q.p1, q.p2);
    } else C = q.pa;
    C *= 1.0 / (4.0 * kPi);
    m22 m;
    m.vv = C * fvv * fvv; m.vh = C * fvh * fvh; m.hv = C * fhv * fhv; m.hh = C * fhh * fhh;
    return m;
}

// cosine in a medium of permittivity e of the direction that has the cosine mu0 in the air (Snell, core/fresnel.py)
SMRT_DEV double fo_snell_from_air(cplx e, double mu0) {
    return csqrt_(cmk(e.re - (1.0 - mu0 * mu0), e.im)).re / csqrt_(e).re;
}

// one boundary seen from above: specular reflection, coherent transmission downwards, diffuse backscatter
struct FoBoundary { double rv, rh, tv, th; m22 bs; };

SMRT_DEV void first_order_angle_item(const FoBatch& b, long long i, int t) {
    const long long gp = fo_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const int L = b.n_layers[s];
    const int nt = b.n_theta;
    double* out = b.out + (i * 4 * nt + t) * 4;                 // + c * nt * 4 for contribution c
    double* lb = b.layer_backscatter ? b.layer_backscatter + (i * (b.Lmax + 1) * nt + t) * 4 : nullptr;   // + (l + 1) * nt * 4
    int bad = 0;
    for (int l = 0; l < L; ++l) if (fo_stage(b, FO_KIND, l, i) < 0.0) bad = 1;
    const double mu0 = cos(b.theta[t]);
    if (!(mu0 > 0.0 && mu0 <= 1.0)) bad = 1;
    if (bad) {
        for (int c = 0; c < 4; ++c) for (int k = 0; k < 4; ++k) out[c * nt * 4 + k] = NAN;
        if (lb) for (int l = 0; l <= b.Lmax; ++l) for (int k = 0; k < 4; ++k) lb[l * nt * 4 + k] = NAN;
        if (t == 0) {
            b.status[i] = ST_INPUT;
            if (b.diag) { b.diag[2 * i] = NAN; b.diag[2 * i + 1] = NAN; }
        }
        return;
    }
    const int* slots = b.itf_slot ? b.itf_slot + gp * (b.Lmax + 1) : nullptr;
    // values of the host-evaluated boundary in slot k at this angle
#define FO_SLOT(k) (b.itf_values + ((gp * b.n_slots + (k)) * nt + t) * kFoInterfaceDoubles)
    m22 acc[4];
    for (int c = 0; c < 4; ++c) acc[c] = m22_zero();
    // the surface: backscatter of a rough surface, coherent transmission into the first layer
    cplx e_l = cmk(fo_stage(b, FO_EPS_RE, 0, i), fo_stage(b, FO_EPS_IM, 0, i));
    double mu_l = fo_snell_from_air(e_l, mu0);
    m22 I;   // downward intensity in the layer for a unit incident intensity
    {
        double tv, th;
        const int k = slots ? slots[0] : -1;
        if (k >= 0) {
            const double* h = FO_SLOT(k);
            tv = h[2]; th = h[3];
            acc[0].vv = h[6]; acc[0].vh = h[7]; acc[0].hv = h[8]; acc[0].hh = h[9];
        } else {
            double rv, rh;
            fresnel_RvRh(cmk(1.0, 0.0), e_l, mu0, &rv, &rh);
            tv = 1.0 - rv; th = 1.0 - rh;
        }
        const double refraction = (1.0 / e_l.re) * (mu0 / mu_l);
        I.vv = tv * refraction; I.hh = th * refraction; I.vh = I.hv = 0.0;
        if (lb) { lb[0] = acc[0].vv * mu0 * 4.0 * kPi; lb[1] = acc[0].vh * mu0 * 4.0 * kPi; lb[2] = acc[0].hv * mu0 * 4.0 * kPi; lb[3] = acc[0].hh * mu0 * 4.0 * kPi; }
    }
    double upv = 1.0, uph = 1.0;   // cumulative upward transmission from the top of layer l to the air
    double albedo_max = 0.0, tau_total = 0.0;
    cplx e_up = cmk(1.0, 0.0);     // medium above layer l
    for (int l = 0; l < L; ++l) {
        const double ks = fo_stage(b, FO_KS, l, i), ka = fo_stage(b, FO_KA, l, i), thick = fo_stage(b, FO_THICK, l, i);
        const int kind = (int)fo_stage(b, FO_KIND, l, i);
        FoLayerPhase q;
        q.phase = kind & 15; q.ms = kind >> 4;
        q.pa = fo_stage(b, FO_PA, l, i); q.pb = fo_stage(b, FO_PB, l, i);
        q.fv = fo_stage(b, FO_FV, l, i); q.p1 = fo_stage(b, FO_P1, l, i); q.p2 = fo_stage(b, FO_P2, l, i);
        // upward coherent transmission through the interface on top of this layer
        {
            const int k = slots ? slots[l] : -1;
            if (k >= 0) { const double* h = FO_SLOT(k); upv *= h[4]; uph *= h[5]; }
            else {
                double rv, rh;
                fresnel_RvRh(e_l, e_up, mu_l, &rv, &rh);
                upv *= 1.0 - rv; uph *= 1.0 - rh;
            }
        }
        if (b.carry) {
            double* c = b.carry + ((i * b.Lmax + l) * nt + t) * kFoCarryDoubles;
            c[0] = I.vv; c[1] = I.hh; c[2] = upv; c[3] = uph; c[4] = mu_l;
        }
        // the boundary below: the next interface, the substrate, or nothing
        FoBoundary bot;
        bot.rv = bot.rh = bot.tv = bot.th = 0.0; bot.bs = m22_zero();
        cplx e_dn = e_l; double mu_dn = mu_l;
        {
            const int k = slots ? slots[l + 1] : -1;
            if (l < L - 1) {
                e_dn = cmk(fo_stage(b, FO_EPS_RE, l + 1, i), fo_stage(b, FO_EPS_IM, l + 1, i));
                mu_dn = fo_snell_from_air(e_dn, mu0);
            }
            if (k >= 0) {
                const double* h = FO_SLOT(k);
                bot.rv = h[0]; bot.rh = h[1];
                if (l < L - 1) { bot.tv = h[2]; bot.th = h[3]; }
                bot.bs.vv = h[6]; bot.bs.vh = h[7]; bot.bs.hv = h[8]; bot.bs.hh = h[9];
            } else if (l < L - 1) {
                fresnel_RvRh(e_l, e_dn, mu_l, &bot.rv, &bot.rh);
                bot.tv = 1.0 - bot.rv; bot.th = 1.0 - bot.rh;
            } else if (b.sub_kind == SUB_FLAT) {
                fresnel_RvRh(e_l, cmk(b.sub_p1[gp], b.sub_p2[gp]), mu_l, &bot.rv, &bot.rh);
            } else if (b.sub_kind == SUB_REFLECTOR) {
                bot.rv = b.sub_p1[gp]; bot.rh = b.sub_p2[gp];
            }
        }
        // the four samples of the phase matrix / 4 pi
        m22 p_up, p_down, p_bi_up, p_bi_down;
        if (q.phase == EM_HOST) {
            if (b.host_phase && ks != 0.0) {
                const double* h = b.host_phase + ((gp * b.Lmax + l) * nt + t) * 16;
                const double c = 1.0 / (4.0 * kPi);
                p_up.vv = c * h[0]; p_up.vh = c * h[1]; p_up.hv = c * h[2]; p_up.hh = c * h[3];
                p_down.vv = c * h[4]; p_down.vh = c * h[5]; p_down.hv = c * h[6]; p_down.hh = c * h[7];
                p_bi_up.vv = c * h[8]; p_bi_up.vh = c * h[9]; p_bi_up.hv = c * h[10]; p_bi_up.hh = c * h[11];
                p_bi_down.vv = c * h[12]; p_bi_down.vh = c * h[13]; p_bi_down.hv = c * h[14]; p_bi_down.hh = c * h[15];
            } else p_up = p_down = p_bi_up = p_bi_down = m22_zero();
        } else if (q.phase == EM_NONSCAT || ks == 0.0) {
            p_up = p_down = p_bi_up = p_bi_down = m22_zero();
        } else {
            p_up = fo_phase(q, -mu_l, mu_l);        // downward -> upward: the volume backscatter
            p_down = fo_phase(q, mu_l, -mu_l);      // upward -> downward
            p_bi_up = fo_phase(q, mu_l, mu_l);      // upward -> upward, bistatic at azimuth pi
            p_bi_down = fo_phase(q, -mu_l, -mu_l);
        }
        const double ke = ks + ka, tau = ke * thick;
        tau_total += tau;
        if (ke > 0.0 && ks / ke > albedo_max) albedo_max = ks / ke;
        const double x = -2.0 * tau / mu_l;
        const double g2 = exp(x);                                      // two-way attenuation
        const double emission = ke > 0.0 ? -expm1(x) / (2.0 * ke) : thick / mu_l;   // (1 - g2) / (2 ke), exact for thin layers
        // order 0: the backscatter of the lower boundary, attenuated
        m22 c0 = m22_left(upv, uph, m22_scale(m22_mul(bot.bs, I), g2));
        // order 1: volume backscatter; one volume scattering and one specular reflection; backscatter between two reflections
        m22 c1 = m22_left(upv, uph, m22_scale(m22_mul(p_up, I), emission));
        m22 bounce = m22_add(m22_right(p_bi_down, bot.rv, bot.rh), m22_left(bot.rv, bot.rh, p_bi_up));
        m22 c2 = m22_left(upv, uph, m22_scale(m22_mul(bounce, I), thick * g2 / mu_l));
        m22 refl = m22_left(bot.rv, bot.rh, m22_right(p_down, bot.rv, bot.rh));
        m22 c3 = m22_left(upv, uph, m22_scale(m22_mul(refl, I), emission * g2));
        acc[0] = m22_add(acc[0], c0); acc[1] = m22_add(acc[1], c1); acc[2] = m22_add(acc[2], c2); acc[3] = m22_add(acc[3], c3);
        if (lb) {
            const double f = mu_l * 4.0 * kPi;
            double* o = lb + (l + 1) * nt * 4;
            o[0] = (c0.vv + c1.vv + c2.vv + c3.vv) * f; o[1] = (c0.vh + c1.vh + c2.vh + c3.vh) * f;
            o[2] = (c0.hv + c1.hv + c2.hv + c3.hv) * f; o[3] = (c0.hh + c1.hh + c2.hh + c3.hh) * f;
        }
        if (l < L - 1) {
            const double f = g2 * (e_l.re / e_dn.re) * (mu_l / mu_dn);   // refraction factor; the reference attenuates the downward intensity by the TWO-way factor here: kept
            I = m22_left(bot.tv, bot.th, m22_scale(I, f));
            e_up = e_l; e_l = e_dn; mu_l = mu_dn;
        }
    }
#undef FO_SLOT
    if (lb) for (int l = L + 1; l <= b.Lmax; ++l) for (int k = 0; k < 4; ++k) lb[l * nt * 4 + k] = 0.0;
    for (int c = 0; c < 4; ++c) {
        double* o = out + c * nt * 4;
        o[0] = acc[c].vv; o[1] = acc[c].vh; o[2] = acc[c].hv; o[3] = acc[c].hh;
    }
    if (t == 0) {
        b.status[i] = ST_OK;
        if (b.diag) { b.diag[2 * i] = albedo_max; b.diag[2 * i + 1] = tau_total; }
    }
}

}  // namespace smrt
