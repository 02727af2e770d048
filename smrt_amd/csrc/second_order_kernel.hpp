// Iterative second-order backscatter solver (the reference's smrt/rtsolver/iterative_second_order.py; Karam et al. 1995
// eqs. A8, A11, A13, azimuth integral by Fourier modes as in Tsang et al. 2007, appendix 2): the per-item arithmetic of
// its kernels.  Orders 0 and 1 are the first-order kernels (first_order_kernel.hpp), which also leave, per (pair, layer,
// angle), the state the order-2 terms are applied to (FoBatch::carry).
//
//   second_order_stream_item    one (pair, layer): the layer's stream set -- Gauss-Legendre nodes of the most refringent
//                               layer carried over by Snell's law, total reflections dropped, finite-difference weights --,
//                               stored ascending (the reference reverses its stream sets).
//   second_order_integral_unit  one WAVEFRONT per (pair, layer, angle) -- double scattering inside the layer and volume
//                               scattering x diffuse reflection of the substrate -- or per (pair, layer n, layer m, angle)
//                               -- double scattering between two layers.  The streams are spread over the lanes; a lane
//                               evaluates, for its stream, the azimuth modes of the left phase matrix of a product (IBA: ALL
//                               modes from one pass over the azimuth samples, the cosines / sines of m phi by rotation;
//                               Rayleigh family: closed forms), contracts them with the right matrix in one more pass (the
//                               right modes are never stored), and applies the closed-form attenuation factor; the weighted
//                               sum over the streams is a wavefront reduction.  The mode count M is a template parameter: the
//                               mode table is indexed by unrolled constants and lives in registers.
//   second_order_walk_item      one (pair, angle): from the surface down, applies the carried downward intensity and
//                               cumulative upward transmission to the integrals, writes the three order-2 contributions
//                               next to the four of the first order, and backscatter_layer = order 1 + order 2.
//
// Only the V, H block of every product is formed: the incident beam has no third Stokes component, the coherent
// interfaces are diagonal and the result is cut to V, H, so of a left factor the rows V, H and of a right factor the columns
// V, H are all that is read.
#pragma once
#include "dort_phase_kernel.hpp"
#include "first_order_kernel.hpp"

namespace smrt {

constexpr int kSo2MaxModes = 8;      // m_max: modes 0 .. m_max - 1 are summed
constexpr int kSo2SubDoubles = 12;   // per (stream, mode) of the substrate's diffuse reflection: rows V, H of two 3 x 3 samples

struct So2Batch {
    FoBatch fo;                      // inputs, staging rows and outputs of the first-order kernels
    int nmax, m_max, nsamp, interlayer;
    long long chunk_begin, chunk_count;   // rows of this launch's chunk; the chunk buffers are indexed by row - chunk_begin
    const double* gl_mu;             // [nmax] positive Gauss-Legendre nodes, descending
    const double* sub_modes;         // [F * S][Lmax][n_theta][nmax][m_max][2][2][3] or null (include/smrt_dort.h)
    int* nstream;                    // chunk: [Lmax]
    double* streams;                 // chunk: [Lmax][2][nmax] ascending cosines, their weights
    double* integ;                   // chunk: [Lmax][n_theta][slots][4], slot 0 intralayer, 1 substrate, 2 + m interlayer with layer m
    double* out;                     // [n_pairs][7][n_theta][2][2]
    double* layer_backscatter;       // [n_pairs][Lmax + 1][n_theta][2][2]
};

SMRT_DEV int so2_slots(const So2Batch& b) { return 2 + (b.interlayer ? b.fo.Lmax : 0); }
SMRT_DEV double* so2_integ(const So2Batch& b, long long r, int l, int t, int slot) {
    return b.integ + (((r * b.fo.Lmax + l) * b.fo.n_theta + t) * so2_slots(b) + slot) * 4;
}

// ---- the stream sets ---------------------------------------------------------------------------------------------------
SMRT_DEV double so2_stream_mu(const So2Batch& b, double ri, int j) {
    const double m = b.gl_mu[j], rs = ri * sqrt(1.0 - m * m);
    return sqrt(1.0 - rs * rs);
}

SMRT_DEV void second_order_stream_item(const So2Batch& b, long long r, int l) {
    const FoBatch& f = b.fo;
    const long long i = b.chunk_begin + r;
    const int L = f.n_layers[(int)(fo_global_pair(f, i) % f.S)];
    int* ns_out = b.nstream + r * f.Lmax + l;
    *ns_out = 0;
    if (l >= L) return;
    int star = 0;   // the most refringent layer (np.argmax on complex: first maximum, real part first)
    for (int k = 0; k < L; ++k) {
        if (fo_stage(f, FO_KIND, k, i) < 0.0) return;   // an invalid layer (status set by first order): no streams, the walk writes NaN
        const double re = fo_stage(f, FO_EPS_RE, k, i), im = fo_stage(f, FO_EPS_IM, k, i);
        const double re0 = fo_stage(f, FO_EPS_RE, star, i), im0 = fo_stage(f, FO_EPS_IM, star, i);
        if (re > re0 || (re == re0 && im > im0)) star = k;
    }
    const cplx es = cmk(fo_stage(f, FO_EPS_RE, star, i), fo_stage(f, FO_EPS_IM, star, i));
    const cplx el = cmk(fo_stage(f, FO_EPS_RE, l, i), fo_stage(f, FO_EPS_IM, l, i));
    const double ri = csqrt_(cdiv(es, el)).re;
    int ns = 0;
    for (int j = 0; j < b.nmax; ++j) {
        const double m = b.gl_mu[j];
        ns += (ri * sqrt(1.0 - m * m) < 1.0) ? 1 : 0;
    }
    if (ns < 2) {   // the reference cannot weight fewer than two streams either
        // Set here, not in the walk: the walk's lanes of one pair (one per angle) all READ the status.  The lanes of one pair
        // here (one per layer) may store concurrently, but only this one value and only over ST_OK.
        if (f.status[i] == ST_OK) f.status[i] = ST_INPUT;
        return;
    }
    double* mu = b.streams + (r * f.Lmax + l) * 2 * b.nmax;
    double* w = mu + b.nmax;
    // the kept streams are the first ns nodes (the relative sine grows with the node index); stored in reverse
    for (int j = 0; j < ns; ++j) {
        double wj;
        if (j == 0) wj = 1.0 - 0.5 * (so2_stream_mu(b, ri, 0) + so2_stream_mu(b, ri, 1));
        else if (j == ns - 1) wj = 0.5 * (so2_stream_mu(b, ri, ns - 2) + so2_stream_mu(b, ri, ns - 1));
        else wj = 0.5 * (so2_stream_mu(b, ri, j - 1) - so2_stream_mu(b, ri, j + 1));
        mu[ns - 1 - j] = so2_stream_mu(b, ri, j);
        w[ns - 1 - j] = fabs(wj);
    }
    *ns_out = ns;
}

// ---- the closed-form factors -------------------------------------------------------------------------------------------
// Each divides by a difference of the two cosines; at exact equality (0 / 0 in the reference) the analytic limit is taken.
SMRT_DEV double so2_coef_A(double mi, double mu, double ke, double tau) {
    const double gi = exp(-tau / mi), gm = exp(-tau / mu);
    const double ratio = mu == mi ? -tau * gi : (gi - gm) / (1.0 / mi - 1.0 / mu);
    return gi * (ratio / ke + mi / (2.0 * ke) * (1.0 - gi * gi)) / (ke * (mi + mu));
}
SMRT_DEV double so2_coef_B(double mi, double mu, double ke, double tau) {
    const double gi = exp(-tau / mi), gm = exp(-tau / mu);
    const double ratio = mu == mi ? -tau * gi : (gm - gi) / (1.0 / mu - 1.0 / mi);
    return (mi * (1.0 - gi * gi) / (2.0 * ke) + gi * ratio / ke) / (ke * (mu + mi));
}
SMRT_DEV double so2_coef_C(double mi, double mu, double ke_n, double ke_m, double tau_n, double tau_m, double tau_r) {
    const double gin = exp(-tau_n / mi), gim = exp(-tau_m / mi), gmn = exp(-tau_n / mu), gmm = exp(-tau_m / mu);
    const double ratio = mu == mi ? -tau_m * gim : (gmm - gim) / (1.0 / mu - 1.0 / mi);
    return gmn * (1.0 - gin * gmn) / (ke_n * (mu + mi)) * ratio / ke_m * exp(-tau_r / mi) * exp(-tau_r / mu);
}
// D = F(mu) G(mu) / (mi - mu)^2 with F = g_m(mi) - g_m(mu) -> 0 and G regular: a simple pole at mu = mi.  There: the finite
// part of its Laurent expansion, -(F'' G / 2 + F' G'), which is the limit of the mean of the two neighbours.
SMRT_DEV double so2_coef_D(double mi, double mu, double ke_n, double ke_m, double tau_n, double tau_m, double tau_r) {
    const double gin = exp(-tau_n / mi), gim = exp(-tau_m / mi);
    if (mu == mi) {
        const double a = mi, gr = exp(-tau_r / mi), k = gim * gr / (ke_n * ke_m);
        const double f1 = gim * tau_m / (a * a);
        const double f2 = gim * (tau_m * tau_m / (a * a * a * a) - 2.0 * tau_m / (a * a * a));
        const double G = k * a * a * (1.0 - gin * gin) * gr;
        const double G1 = k * a * gr * ((1.0 - gin * gin) - gin * gin * tau_n / a + (1.0 - gin * gin) * tau_r / a);
        return -(f2 * G / 2.0 + f1 * G1);
    }
    const double gmn = exp(-tau_n / mu), gmm = exp(-tau_m / mu);
    return (gim - gmm) / (ke_m * (mi - mu)) * gim * (1.0 - gmn * gin) / (ke_n * (1.0 / mu - 1.0 / mi)) * exp(-tau_r / mi) *
           exp(-tau_r / mu);
}
SMRT_DEV double so2_coef_F(double mi, double mu, double ke, double tau, double tau_ground) {
    const double gi = exp(-tau / mi), gm = exp(-tau / mu);
    const double ratio = mu == mi ? gi * tau / (mi * mi) : (gm - gi) / (mu - mi);
    return gi * mi * ratio / ke * exp(-tau_ground / mi) * exp(-tau_ground / mu);
}
SMRT_DEV double so2_coef_E(double mi, double mu, double ke, double tau, double tau_ground) {
    return exp(-tau / mi) * so2_coef_F(mi, mu, ke, tau, tau_ground);
}

// ---- azimuth modes of the phase matrices -----------------------------------------------------------------------------------
// Of a LEFT factor the product reads the rows V, H: d[m] = (vv, vh, hv, hh) and x[m] = (e[V][U], e[H][U]); of a RIGHT factor
// the columns V, H: the same block and (e[U][V], e[U][H]).  Nothing here is divided by 4 pi.
struct So2Sample { double b0, b1, b2, b3, y0, y1; };
// IBA's phase matrix at one azimuth (the sampled function of ft_even_phase_mode)
template <bool LEFT>
SMRT_DEV So2Sample so2_iba_sample(const FoLayerPhase& q, double mu_s, double mu_i, double ss, double si, double c, double sn) {
    double ct = mu_s * mu_i + ss * si * c;
    ct = ct > 1.0 ? 1.0 : (ct < -1.0 ? -1.0 : ct);
    double C;
    if (q.ms == MS_EXP) { const double dp = 1.0 + q.pb * (1.0 - ct); C = q.pa / (dp * dp); }
    else C = q.pa * ft_corr(q.ms, q.pb * (1.0 - ct), q.fv, q.p1, q.p2);
    const double fvv = c * mu_s * mu_i + ss * si, fvh = sn * mu_s, fhv = -sn * mu_i, fhh = c;
    So2Sample r;
    r.b0 = fvv * fvv * C; r.b1 = fvh * fvh * C; r.b2 = fhv * fhv * C; r.b3 = fhh * fhh * C;
    r.y0 = LEFT ? -fvh * fvv * C : 2.0 * fvv * fhv * C; r.y1 = LEFT ? -fhh * fhv * C : 2.0 * fvh * fhh * C;
    return r;
}

// Modes 0 .. M - 1 of a LEFT factor.  IBA: every mode from ONE pass over the samples of [0, pi], cos(m phi) / sin(m phi) by
// rotation; Rayleigh family: closed forms, modes 0 .. 2.
template <int M>
SMRT_DEV void so2_left_modes(const FoLayerPhase& q, double mu_s, double mu_i, int nsamp, double (&d)[M][4], double (&x)[M][2]) {
#pragma unroll
    for (int m = 0; m < M; ++m) { d[m][0] = d[m][1] = d[m][2] = d[m][3] = 0.0; x[m][0] = x[m][1] = 0.0; }
    if (q.phase == EM_NONSCAT) return;
    if (q.phase != EM_IBA) {
#pragma unroll
        for (int m = 0; m < M && m < 3; ++m) {
            double e[3][3];
            ft_even_phase_mode(EM_DMRT, q.ms, q.pa, q.pb, q.fv, q.p1, q.p2, mu_s, mu_i, m, 3, nsamp, e);
            d[m][0] = e[0][0]; d[m][1] = e[0][1]; d[m][2] = e[1][0]; d[m][3] = e[1][1];
            x[m][0] = e[0][2]; x[m][1] = e[1][2];
        }
        return;
    }
    const double ss = sqrt(1.0 - mu_s * mu_s), si = sqrt(1.0 - mu_i * mu_i);
    const int nphi = nsamp / 2 + 1;
    const double inv = 1.0 / (double)nsamp;
    for (int k = 0; k < nphi; ++k) {
        const double ph = kPi * (double)k / (double)(nphi - 1);
        const double c = cos(ph), sn = sin(ph);
        const bool end = (k == 0 || k == nphi - 1);
        const So2Sample p = so2_iba_sample<true>(q, mu_s, mu_i, ss, si, c, sn);
        const double wc = (end ? 1.0 : 2.0) * inv, ws = end ? 0.0 : 2.0 * inv;
        double cm = 1.0, sm = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double base = m == 0 ? 1.0 : 2.0;
            const double cw = base * wc * cm, sw = base * ws * sm;
            d[m][0] += p.b0 * cw; d[m][1] += p.b1 * cw; d[m][2] += p.b2 * cw; d[m][3] += p.b3 * cw;
            x[m][0] += p.y0 * sw; x[m][1] += p.y1 * sw;
            const double cn = cm * c - sm * sn;
            sm = sm * c + cm * sn; cm = cn;
        }
    }
}

// s += f * sum_m w_m (left_m right_m)[V, H block], w_0 = 2 pi, w_m = pi cos(m pi), modes below m_max only; the RIGHT factor
// is the phase matrix of q between (mu_s, mu_i).  Its modes are never stored: per azimuth sample the left table is
// contracted over the modes first, so the only table a lane holds is the left one.
template <int M>
SMRT_DEV void so2_add_products(double (&s)[4], double f, int m_max, const double (&ld)[M][4], const double (&lx)[M][2],
                               const FoLayerPhase& q, double mu_s, double mu_i, int nsamp) {
    if (q.phase == EM_NONSCAT) return;
    if (q.phase != EM_IBA) {
#pragma unroll
        for (int m = 0; m < M && m < 3; ++m) {
            double e[3][3];
            ft_even_phase_mode(EM_DMRT, q.ms, q.pa, q.pb, q.fv, q.p1, q.p2, mu_s, mu_i, m, 3, nsamp, e);
            const double w = m >= m_max ? 0.0 : f * (m == 0 ? 2.0 * kPi : ((m & 1) ? -kPi : kPi));
            s[0] += w * (ld[m][0] * e[0][0] + ld[m][1] * e[1][0] + lx[m][0] * e[2][0]);
            s[1] += w * (ld[m][0] * e[0][1] + ld[m][1] * e[1][1] + lx[m][0] * e[2][1]);
            s[2] += w * (ld[m][2] * e[0][0] + ld[m][3] * e[1][0] + lx[m][1] * e[2][0]);
            s[3] += w * (ld[m][2] * e[0][1] + ld[m][3] * e[1][1] + lx[m][1] * e[2][1]);
        }
        return;
    }
    const double ss = sqrt(1.0 - mu_s * mu_s), si = sqrt(1.0 - mu_i * mu_i);
    const int nphi = nsamp / 2 + 1;
    const double inv = f / (double)nsamp;
    for (int k = 0; k < nphi; ++k) {
        const double ph = kPi * (double)k / (double)(nphi - 1);
        const double c = cos(ph), sn = sin(ph);
        const bool end = (k == 0 || k == nphi - 1);
        const So2Sample p = so2_iba_sample<false>(q, mu_s, mu_i, ss, si, c, sn);
        const double wc = (end ? 1.0 : 2.0) * inv, ws = end ? 0.0 : 2.0 * inv;
        double cm = 1.0, sm = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, u0 = 0.0, u1 = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double w = m >= m_max ? 0.0 : (m == 0 ? 2.0 * kPi : ((m & 1) ? -2.0 * kPi : 2.0 * kPi));   // w_m x (1 or 2)
            const double cw = w * wc * cm, sw = w * ws * sm;
            t0 += cw * ld[m][0]; t1 += cw * ld[m][1]; t2 += cw * ld[m][2]; t3 += cw * ld[m][3];
            u0 += sw * lx[m][0]; u1 += sw * lx[m][1];
            const double cn = cm * c - sm * sn;
            sm = sm * c + cm * sn; cm = cn;
        }
        s[0] += t0 * p.b0 + t1 * p.b2 + u0 * p.y0;
        s[1] += t0 * p.b1 + t1 * p.b3 + u0 * p.y1;
        s[2] += t2 * p.b0 + t3 * p.b2 + u1 * p.y0;
        s[3] += t2 * p.b1 + t3 * p.b3 + u1 * p.y1;
    }
}

SMRT_DEV FoLayerPhase so2_layer_phase(const FoBatch& f, long long i, int l) {
    const int kind = (int)fo_stage(f, FO_KIND, l, i);
    FoLayerPhase q;
    q.phase = kind & 15; q.ms = kind >> 4;
    q.pa = fo_stage(f, FO_PA, l, i); q.pb = fo_stage(f, FO_PB, l, i);
    q.fv = fo_stage(f, FO_FV, l, i); q.p1 = fo_stage(f, FO_P1, l, i); q.p2 = fo_stage(f, FO_P2, l, i);
    if (fo_stage(f, FO_KS, l, i) == 0.0) q.phase = EM_NONSCAT;
    return q;
}

// One wavefront: `lane` 0 .. 63.  m < 0: the (pair, layer n, angle) unit -- slots 0 and 1; else the interlayer unit (n, m).
template <int M>
SMRT_DEV void second_order_integral_unit(const So2Batch& b, long long r, int n, int m, int t, int lane) {
    const FoBatch& f = b.fo;
    const long long i = b.chunk_begin + r;
    const long long gp = fo_global_pair(f, i);
    const int L = f.n_layers[(int)(gp % f.S)];
    if (n >= L || m >= L || (m >= 0 && m <= n)) return;   // never read by the walk
    const int ns_n = b.nstream[r * f.Lmax + n];
    const int ns_m = m < 0 ? ns_n : b.nstream[r * f.Lmax + m];
    const int ns = ns_m < ns_n ? ns_m : ns_n;
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
    const FoLayerPhase qn = so2_layer_phase(f, i, n);
    const double mu0 = cos(f.theta[t]);
    const double mi = fo_snell_from_air(cmk(fo_stage(f, FO_EPS_RE, n, i), fo_stage(f, FO_EPS_IM, n, i)), mu0);
    const double ke_n = fo_stage(f, FO_KS, n, i) + fo_stage(f, FO_KA, n, i), tau_n = ke_n * fo_stage(f, FO_THICK, n, i);
    const double* mu_n = b.streams + (r * f.Lmax + n) * 2 * b.nmax;
    const double* w_n = mu_n + b.nmax;
    const double c16 = 1.0 / (16.0 * kPi * kPi), c4 = 1.0 / (4.0 * kPi);
    double ld[M][4], lx[M][2];
    if (m < 0) {
        const bool scatters = qn.phase != EM_NONSCAT && ns_n > 0;
        double tau_ground = 0.0;
        for (int k = n; k < L; ++k) tau_ground += (fo_stage(f, FO_KS, k, i) + fo_stage(f, FO_KA, k, i)) * fo_stage(f, FO_THICK, k, i);
        for (int j = lane; scatters && j < ns; j += SMRT_LANES) {
            const double x = mu_n[j], w = w_n[j];
            so2_left_modes<M>(qn, mi, x, b.nsamp, ld, lx);                                                          // P(mu_i <- mu')
            so2_add_products<M>(s0, w * c16 * so2_coef_A(mi, x, ke_n, tau_n), b.m_max, ld, lx, qn, x, -mi, b.nsamp);    // P(mu' <- -mu_i)
            so2_left_modes<M>(qn, mi, -x, b.nsamp, ld, lx);                                                         // P(mu_i <- -mu')
            so2_add_products<M>(s0, w * c16 * so2_coef_B(mi, x, ke_n, tau_n), b.m_max, ld, lx, qn, -x, -mi, b.nsamp);   // P(-mu' <- -mu_i)
            if (b.sub_modes) {
                const double* h = b.sub_modes + ((((gp * f.Lmax + n) * f.n_theta + t) * b.nmax + j) * b.m_max) * kSo2SubDoubles;
                // R(-mu_i <- mu') P(-mu' <- -mu_i), then R(mu' <- mu_i) P(mu_i <- mu')
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    const double* g = h + (k < b.m_max ? k : 0) * kSo2SubDoubles;
                    ld[k][0] = g[0]; ld[k][1] = g[1]; lx[k][0] = g[2]; ld[k][2] = g[3]; ld[k][3] = g[4]; lx[k][1] = g[5];
                }
                so2_add_products<M>(s1, w * c4 * so2_coef_E(mi, x, ke_n, tau_n, tau_ground), b.m_max, ld, lx, qn, -x, -mi, b.nsamp);
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    const double* g = h + (k < b.m_max ? k : 0) * kSo2SubDoubles + 6;
                    ld[k][0] = g[0]; ld[k][1] = g[1]; lx[k][0] = g[2]; ld[k][2] = g[3]; ld[k][3] = g[4]; lx[k][1] = g[5];
                }
                so2_add_products<M>(s1, w * c4 * so2_coef_F(mi, x, ke_n, tau_n, tau_ground), b.m_max, ld, lx, qn, mi, x, b.nsamp);
            }
        }
    } else {
        const FoLayerPhase qm = so2_layer_phase(f, i, m);
        const bool scatters = qn.phase != EM_NONSCAT && qm.phase != EM_NONSCAT;
        const double mm = fo_snell_from_air(cmk(fo_stage(f, FO_EPS_RE, m, i), fo_stage(f, FO_EPS_IM, m, i)), mu0);
        const double ke_m = fo_stage(f, FO_KS, m, i) + fo_stage(f, FO_KA, m, i), tau_m = ke_m * fo_stage(f, FO_THICK, m, i);
        double tau_r = tau_n;   // both end layers and everything between them, as the reference accumulates it
        for (int k = n + 1; k <= m; ++k) tau_r += (fo_stage(f, FO_KS, k, i) + fo_stage(f, FO_KA, k, i)) * fo_stage(f, FO_THICK, k, i);
        const double* mu_m = b.streams + (r * f.Lmax + m) * 2 * b.nmax;
        for (int j = lane; scatters && j < ns; j += SMRT_LANES) {
            const double x = mu_n[j], w = w_n[j], y = mu_m[j];
            so2_left_modes<M>(qn, mi, x, b.nsamp, ld, lx);      // layer n: P(mu_i <- mu'); layer m: P(mu' <- -mu_i)
            so2_add_products<M>(s0, w * c16 * so2_coef_C(mi, x, ke_n, ke_m, tau_n, tau_m, tau_r), b.m_max, ld, lx, qm, y, -mm, b.nsamp);
            so2_left_modes<M>(qm, mm, -y, b.nsamp, ld, lx);     // layer m: P(mu_i <- -mu'); layer n: P(-mu' <- -mu_i)
            so2_add_products<M>(s0, w * c16 * so2_coef_D(mi, x, ke_n, ke_m, tau_n, tau_m, tau_r), b.m_max, ld, lx, qn, -x, -mi, b.nsamp);
        }
    }
    for (int k = 0; k < 4; ++k) s0[k] = group_sum<SMRT_LANES>(s0[k]);
    if (m < 0) for (int k = 0; k < 4; ++k) s1[k] = group_sum<SMRT_LANES>(s1[k]);
    if (lane == 0) {
        double* o = so2_integ(b, r, n, t, m < 0 ? 0 : 2 + m);
        o[0] = s0[0]; o[1] = s0[1]; o[2] = s0[2]; o[3] = s0[3];
        if (m < 0) { o[4] = s1[0]; o[5] = s1[1]; o[6] = s1[2]; o[7] = s1[3]; }
    }
}

// ---- the walk: one (pair, incidence angle) -------------------------------------------------------------------------------
SMRT_DEV void second_order_walk_item(const So2Batch& b, long long r, int t) {
    const FoBatch& f = b.fo;
    const long long i = b.chunk_begin + r;
    const int L = f.n_layers[(int)(fo_global_pair(f, i) % f.S)];
    const int nt = f.n_theta;
    double* out = b.out + (i * 7 * nt + t) * 4;                                  // + c * nt * 4 for contribution c
    double* lb = b.layer_backscatter + (i * (f.Lmax + 1) * nt + t) * 4;            // + (l + 1) * nt * 4
    const double* fo_out = f.out + (i * 4 * nt + t) * 4;
    const double* fo_lb = f.layer_backscatter + (i * (f.Lmax + 1) * nt + t) * 4;
    for (int c = 0; c < 4; ++c) for (int k = 0; k < 4; ++k) out[c * nt * 4 + k] = fo_out[c * nt * 4 + k];
    for (int l = 0; l <= f.Lmax; ++l) for (int k = 0; k < 4; ++k) lb[l * nt * 4 + k] = fo_lb[l * nt * 4 + k];
    bool bad = f.status[i] != ST_OK;   // first order's, or ST_INPUT from the streams kernel: fewer than two streams in a layer
    for (int l = 0; l < L; ++l) if (b.nstream[r * f.Lmax + l] < 2) bad = true;
    if (bad) {
        for (int c = 4; c < 7; ++c) for (int k = 0; k < 4; ++k) out[c * nt * 4 + k] = NAN;
        for (int l = 1; l <= L; ++l) for (int k = 0; k < 4; ++k) lb[l * nt * 4 + k] = NAN;
        return;
    }
    double intra[4] = {0.0, 0.0, 0.0, 0.0}, ground[4] = {0.0, 0.0, 0.0, 0.0}, inter[4] = {0.0, 0.0, 0.0, 0.0};
    for (int n = 0; n < L; ++n) {
        const double* c = f.carry + ((i * f.Lmax + n) * nt + t) * kFoCarryDoubles;   // I_v, I_h, up_v, up_h, mu in the layer
        const double lr[4] = {c[2] * c[0], c[2] * c[1], c[3] * c[0], c[3] * c[1]};    // diag(up) S diag(I), element by element
        const double* s = so2_integ(b, r, n, t, 0);
        for (int k = 0; k < 4; ++k) { intra[k] += lr[k] * s[k]; ground[k] += lr[k] * s[4 + k]; }
        for (int m = n + 1; b.interlayer && m < L; ++m) {
            const double* u = so2_integ(b, r, n, t, 2 + m);
            for (int k = 0; k < 4; ++k) inter[k] += lr[k] * u[k];
        }
        // the reference's per-layer entry is the RUNNING sum of the two terms, scaled with this layer's cosine: kept
        for (int k = 0; k < 4; ++k) lb[(n + 1) * nt * 4 + k] += (intra[k] + ground[k]) * c[4] * 4.0 * kPi;
    }
    for (int k = 0; k < 4; ++k) { out[4 * nt * 4 + k] = intra[k]; out[5 * nt * 4 + k] = ground[k]; out[6 * nt * 4 + k] = inter[k]; }
}

}  // namespace smrt
