// Successive-order-of-scattering solver, passive mode (the reference's smrt/rtsolver/successive_order.py; Lenoble et al.
// 2007 eq. 66, Greenwald et al. 2005 eq. 2): the per-item arithmetic of its three kernels.
//
//   so_layer_item   one (pair, layer): the layer electromagnetics (layer_em) and the number of sublayers,
//                   max(ceil(ke d / 0.1), 1).  The host reads the sublayer counts back: they size the workspace.
//   so_prep_item    one workgroup per (pair, layer): the streams of the layer (Snell from the most refringent one), per
//                   direction e^(-dtau / mu) and the Fresnel coefficients of the two interfaces of the layer, the source
//                   (1 - omega) B(T), and the weighted phase matrix (1 / ke) 1/2 P0 w of mode 0 on the +-mu grid
//                   (ft_even_phase_mode of dort_phase_kernel.hpp), stored TRANSPOSED and zero-padded to a multiple of 16.
//   so_sweep_pair   one workgroup of 256 threads per pair, all orders in one call.  Per order:
//                     (a) source product S[k][d] = sum_q mean[k][q] Wt[q][d] over the K sublayers of every layer with
//                         v_mfma_f64_16x16x4_f64: the means of 16 sublayers are staged in LDS (A operand), Wt is read
//                         from global memory with unit stride (B operand), four wavefronts share the 16-direction tiles;
//                     (b) the reflections of the previous order at the interfaces (read before the profile is overwritten);
//                     (c) the two recurrences I <- I e + S (1 - e), one lane per direction: threads 0..127 sweep down,
//                         threads 128..255 sweep up, concurrently (neither needs the other's result of the same order);
//                     (d) the emerging radiance, the stopping rule (workgroup-uniform), the order's brightness temperature.
//                   The profile (radiance at every sub-interface, 2 x 2 x n directions) and the source live in a global
//                   workspace; the profile is updated in place.
//
// Direction index inside a layer of n streams: d < 2 n upward (stream d / 2, polarisation d & 1: V, H), 2 n <= d < 4 n
// downward.  The same source is compiled by g++ (-DSMRT_HOST_EMU) for the CPU tests.
#pragma once
#include "dort_phase_kernel.hpp"

namespace smrt {

constexpr int ST_DEPTH = 7;          // the pair does not fit the workspace budget (set by the host, never by a kernel)
constexpr int kSoThreads = 256;
constexpr int kSoMaxStream = 64;     // 2 n <= 128 directions per hemisphere: one lane each in half a workgroup
constexpr double kSoDtau = 0.1;      // optical depth of a sublayer (the reference's infinitesimal_optical_depth)

// staging rows, each [Lmax][n_pairs]
enum { SO_EPS_RE = 0, SO_EPS_IM, SO_KS, SO_KA, SO_PA, SO_PB, SO_KIND, SO_ROWS };
// per (pair, layer) vectors of Dh = 2 n_max_stream doubles
enum { SO_EXT = 0, SO_RTOP, SO_TTOP, SO_RBOT, SO_TBOT, SO_EMIS, SO_VECS };

SMRT_HD int so_round16(int n) { return (n + 15) & ~15; }
SMRT_HD int so_dp(int n_max_stream) { return so_round16(4 * n_max_stream); }                 // stride of a profile row
SMRT_HD int so_tile_ld(int n_max_stream) { return ((so_dp(n_max_stream) + 31) & ~31) + 2; }  // LDS row stride: 2 mod 32, conflict-free A reads
SMRT_HD int so_lds_doubles(int n_max_stream, int n_theta) {
    (void)n_theta;
    return 16 * so_tile_ld(n_max_stream) + 3 * 2 * n_max_stream + n_max_stream + 8;   // tile, emerging / tb / total, air cosines, scalars
}

struct SoBatch {
    int S, Lmax, F, n_theta;
    int emmodel, micro, sub_kind, nmax;
    int n_iter, rj, nsamp, reserved;
    double rtol;
    long long n_pairs;              // pairs of the resident batch (rows of every output)
    long long chunk_begin, chunk_count;   // rows of this launch of so_prep / so_sweep; Wt and the workspace are per chunk
    const long long* pair_map;      // null: row i is pair i of the flattened f * S + s list; else pair pair_map[i]
    const int* n_layers;
    const double *thickness, *frac_volume, *temperature, *p1, *p2, *frequency, *theta, *liquid_water;
    const int* layer_kind;
    const double *sub_p1, *sub_p2;  // [F][S]
    const double* sub_T;            // [S], <= 0: no emission
    const double* gl_mu;            // [nmax] positive Gauss-Legendre nodes, descending
    double* stage;                  // [SO_ROWS][Lmax][n_pairs]
    int* nsub;                      // [n_pairs][Lmax] sublayers (0 below the last layer)
    int* nstream;                   // [n_pairs][Lmax]
    double* vec;                    // [n_pairs][Lmax][SO_VECS][2 nmax]
    double* srcterm;                // [n_pairs][Lmax] (1 - omega) B(T)
    double* wt;                     // [chunk_count][Lmax][Dp][Dp] transposed weighted phase matrix
    const long long* ws_off;        // [n_pairs] offset (doubles) of the pair's workspace inside its chunk's
    double* ws;                     // per pair: profile [I][Dp], source [K][Dp], boundary [Lmax][2][2 nmax]; I, K: sub-interfaces, sublayers of the pair
    double* out;                    // [n_pairs][n_iter + 1][2][n_theta] kelvin; the last row is the total
    int* status;                    // [n_pairs]
    double* layer_out;              // [n_pairs][Lmax][5]: Re eps, Im eps, ks, ka, streams
    double* streams;                // [n_pairs][1 + nmax]: n_air, cosines of the air streams
    double* maxrad;                 // [n_pairs][n_iter] largest emerging radiance of every order run, 0 after the stop
    int* orders;                    // [n_pairs] orders run
};

SMRT_DEV long long so_global_pair(const SoBatch& b, long long i) { return b.pair_map ? b.pair_map[i] : i; }
SMRT_DEV double& so_stage(const SoBatch& b, int row, int l, long long i) {
    return b.stage[((long long)row * b.Lmax + l) * b.n_pairs + i];
}

// ---- kernel (a): one (pair, layer) -------------------------------------------------------------------------------------
SMRT_DEV void so_layer_item(const SoBatch& b, long long i, int l) {
    const long long gp = so_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const double frequency = b.frequency[gp / b.S];
    const int L = b.n_layers[s];
    double* lo = b.layer_out + (i * b.Lmax + l) * 5;
    if (l >= L) {
        so_stage(b, SO_KIND, l, i) = -1.0;
        b.nsub[i * b.Lmax + l] = 0;
        lo[0] = lo[1] = lo[2] = lo[3] = lo[4] = 0.0;
        return;
    }
    const long long at = (long long)s * b.Lmax + l;
    const int kind = b.layer_kind ? b.layer_kind[at] : b.emmodel + 16 * b.micro;
    const int em = kind & 15, ms = kind >> 4;
    cplx ee = cmk(1.0, 0.0); double ks = 0.0, ka = 0.0, pa = 0.0, pb = 0.0; int bad = 0;
    if (em == EM_HOST || em == EM_IBA_HOST || em == EM_RAYLEIGH_HOST || ms >= MS_EXPC) bad = 1;   // emmodels evaluated on the host: not here
    else layer_em(em, ms, frequency, b.frac_volume[at], b.temperature[at], b.p1[at], b.p2 ? b.p2[at] : 0.0, &ee, &ks, &ka, &pa, &pb,
                  &bad, b.liquid_water ? b.liquid_water[at] : 0.0);
    const double thick = b.thickness[at], ke = ks + ka;
    if (!(ks >= 0.0) || !(thick > 0.0) || !(ke > 0.0)) bad = 1;
    const int phase = (em == EM_IBA || em == EM_IBA_INV) ? EM_IBA : em == EM_NONSCAT ? EM_NONSCAT : EM_DMRT;
    so_stage(b, SO_EPS_RE, l, i) = ee.re; so_stage(b, SO_EPS_IM, l, i) = ee.im;
    so_stage(b, SO_KS, l, i) = ks; so_stage(b, SO_KA, l, i) = ka;
    so_stage(b, SO_PA, l, i) = pa; so_stage(b, SO_PB, l, i) = pb;
    so_stage(b, SO_KIND, l, i) = bad ? -2.0 : (double)(phase + 16 * ms);
    int K = 1;
    if (!bad) {
        const double k = ceil(ke * thick / kSoDtau);
        K = k < 1.0 ? 1 : (k > 1.0e9 ? 1000000000 : (int)k);
    }
    b.nsub[i * b.Lmax + l] = K;
    lo[0] = ee.re; lo[1] = ee.im; lo[2] = ks; lo[3] = ka; lo[4] = 0.0;
}

// ---- kernel (b): one workgroup per (pair, layer) ------------------------------------------------------------------------
// relative sine of layer l: sqrt(eps* / eps_l).re, eps* the most refringent layer (np.argmax on complex: first maximum)
SMRT_DEV cplx so_estar(const SoBatch& b, long long i, int L) {
    int k = 0;
    for (int l = 1; l < L; ++l) {
        const double re = so_stage(b, SO_EPS_RE, l, i), im = so_stage(b, SO_EPS_IM, l, i);
        const double re0 = so_stage(b, SO_EPS_RE, k, i), im0 = so_stage(b, SO_EPS_IM, k, i);
        if (re > re0 || (re == re0 && im > im0)) k = l;
    }
    return cmk(so_stage(b, SO_EPS_RE, k, i), so_stage(b, SO_EPS_IM, k, i));
}
SMRT_DEV int so_count_streams(const SoBatch& b, double ri) {
    int n = 0;
    for (int j = 0; j < b.nmax; ++j) {
        const double m = b.gl_mu[j];
        n += (ri * sqrt(1.0 - m * m) < 1.0) ? 1 : 0;
    }
    return n;
}
SMRT_DEV double so_mu(const SoBatch& b, double ri, int j) {
    const double m = b.gl_mu[j], rs = ri * sqrt(1.0 - m * m);
    return sqrt(1.0 - rs * rs);
}
// quadrature weight of stream j of n (streams.py: finite differences of the cosines, absolute value)
SMRT_DEV double so_weight(const SoBatch& b, double ri, int j, int n) {
    double w;
    if (j == 0) w = 1.0 - 0.5 * (so_mu(b, ri, 0) + so_mu(b, ri, 1));
    else if (j == n - 1) w = 0.5 * (so_mu(b, ri, n - 2) + so_mu(b, ri, n - 1));
    else w = 0.5 * (so_mu(b, ri, j - 1) - so_mu(b, ri, j + 1));
    return fabs(w);
}

template <int NT>
SMRT_DEV void so_prep_item(const SoBatch& b, long long i, int l) {
    const int t = tid();
    const long long gp = so_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const int L = b.n_layers[s];
    if (l >= L) return;
    for (int k = 0; k < L; ++k) if (so_stage(b, SO_KIND, k, i) < 0.0) return;   // the sweep kernel reports it
    const double frequency = b.frequency[gp / b.S];
    const cplx estar = so_estar(b, i, L);
    const cplx el = cmk(so_stage(b, SO_EPS_RE, l, i), so_stage(b, SO_EPS_IM, l, i));
    const double ri = csqrt_(cdiv(estar, el)).re;
    const int ns = so_count_streams(b, ri);
    if (t == 0) {
        b.nstream[i * b.Lmax + l] = ns;
        b.layer_out[(i * b.Lmax + l) * 5 + 4] = (double)ns;
    }
    if (ns < 2) return;
    const long long at = (long long)s * b.Lmax + l;
    const double ks = so_stage(b, SO_KS, l, i), ka = so_stage(b, SO_KA, l, i), ke = ks + ka;
    const int K = b.nsub[i * b.Lmax + l];
    const int Dh = 2 * b.nmax, Dp = so_dp(b.nmax);
    const int n = 2 * ns;   // directions per hemisphere
    double* vec = b.vec + (i * b.Lmax + l) * SO_VECS * Dh;
    const double BT = b.rj ? b.temperature[at] : planck_radiance(frequency, b.temperature[at]);
    if (t == 0) b.srcterm[i * b.Lmax + l] = (1.0 - ks * (1.0 / ke)) * BT;
    for (int j = t; j < n; j += NT) {
        const double mu = so_mu(b, ri, j >> 1);
        const int h = j & 1;
        vec[SO_EXT * Dh + j] = exp(-(ke * b.thickness[at]) / (double)K / mu);
        const cplx eup = l > 0 ? cmk(so_stage(b, SO_EPS_RE, l - 1, i), so_stage(b, SO_EPS_IM, l - 1, i)) : cmk(1.0, 0.0);
        double rv, rh;
        fresnel_RvRh(el, eup, mu, &rv, &rh);
        vec[SO_RTOP * Dh + j] = h ? rh : rv;
        vec[SO_TTOP * Dh + j] = 1.0 - (h ? rh : rv);
        double rb = 0.0, tb = 0.0, emis = 0.0;
        if (l < L - 1) {
            fresnel_RvRh(el, cmk(so_stage(b, SO_EPS_RE, l + 1, i), so_stage(b, SO_EPS_IM, l + 1, i)), mu, &rv, &rh);
            rb = h ? rh : rv; tb = 1.0 - rb;
        } else if (b.sub_kind != SUB_NONE) {
            if (b.sub_kind != SUB_REFLECTOR) {   // Flat, or a rough soil
                substrate_RvRh(b, gp, s, frequency, el, mu, &rv, &rh);
                rb = h ? rh : rv;
            } else rb = h ? b.sub_p2[gp] : b.sub_p1[gp];
            const double Ts = b.sub_T ? b.sub_T[s] : 0.0;
            if (Ts > 0.0) emis = (1.0 - rb) * (b.rj ? Ts : planck_radiance(frequency, Ts));   // the substrate's own emission
        }
        vec[SO_RBOT * Dh + j] = rb; vec[SO_TBOT * Dh + j] = tb; vec[SO_EMIS * Dh + j] = emis;
    }
    // the transposed weighted phase matrix: Wt[q][d] = (1 / ke) 1/2 P0[d][q] w_q, zero outside the 4 ns directions
    double* wt = b.wt + ((i - b.chunk_begin) * b.Lmax + l) * (long long)Dp * Dp;
    const int n16 = so_round16(2 * n);
    for (int idx = t; idx < n16 * n16; idx += NT) wt[(long long)(idx / n16) * Dp + idx % n16] = 0.0;
    block_sync();
    const int kind = (int)so_stage(b, SO_KIND, l, i);
    const int em = kind & 15, ms = kind >> 4;
    if (em == EM_NONSCAT || ks == 0.0) return;
    const double pa = so_stage(b, SO_PA, l, i), pb = so_stage(b, SO_PB, l, i);
    const double fv = b.frac_volume[at], p1 = b.p1[at], p2 = b.p2 ? b.p2[at] : 0.0;
    const double invke = 1.0 / ke;
    for (int idx = t; idx < 4 * ns * ns; idx += NT) {
        const int fs = idx / (2 * ns), fi = idx % (2 * ns);   // scattered / incident stream of the full (+mu, -mu) grid
        const int js = fs < ns ? fs : fs - ns, ji = fi < ns ? fi : fi - ns;
        const double mus = fs < ns ? so_mu(b, ri, js) : -so_mu(b, ri, js);
        const double mui = fi < ns ? so_mu(b, ri, ji) : -so_mu(b, ri, ji);
        double e[3][3];
        ft_even_phase_mode(em, ms, pa, pb, fv, p1, p2, mus, mui, 0, 2, b.nsamp, e);
        const double w = so_weight(b, ri, ji, ns);
        const int d0 = (fs < ns ? 0 : n) + 2 * js, q0 = (fi < ns ? 0 : n) + 2 * ji;
        for (int a = 0; a < 2; ++a)
            for (int c = 0; c < 2; ++c)
                wt[(long long)(q0 + c) * Dp + d0 + a] = invke * (0.5 * e[a][c]) * w;
    }
}

// ---- kernel (c): one workgroup per pair ---------------------------------------------------------------------------------
// Linear inter / extrapolation in the cosine to the sensor angles (rtsolver_utils.py:179-239): outmu is descending; a
// virtual node mu = 1 holding the mean of V and H of the steepest stream stands in front of it for a steeper request.
SMRT_DEV double so_interpolate(const double* outmu, const double* tb, int n_air, int pol, double um) {
    double x0, x1, y0, y1;
    const double top = 0.5 * (tb[0] + tb[1]);
    if (um > outmu[0] || n_air == 1) { x0 = 1.0; y0 = top; x1 = outmu[0]; y1 = tb[pol]; }
    else {
        int k = 0;
        while (k < n_air - 2 && um < outmu[k + 1]) ++k;
        x0 = outmu[k]; y0 = tb[2 * k + pol]; x1 = outmu[k + 1]; y1 = tb[2 * (k + 1) + pol];
    }
    return y0 + (y1 - y0) * ((um - x0) / (x1 - x0));
}

template <int NT>
SMRT_DEV void so_sweep_pair(const SoBatch& b, long long i, double* lds) {
    static_assert(NT == 256, "threads 0..127 sweep down, 128..255 sweep up");
    const int t = tid();
    const long long gp = so_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const int L = b.n_layers[s];
    const double frequency = b.frequency[gp / b.S];
    const int Dh = 2 * b.nmax, Dp = so_dp(b.nmax), LDm = so_tile_ld(b.nmax);
    const int NO = b.n_iter, nt = b.n_theta;
    double* out = b.out + i * (long long)(NO + 1) * 2 * nt;
    double* tile = lds;                       // [16][LDm]
    double* emerg = tile + 16 * LDm;          // [Dh]
    double* tbv = emerg + Dh;                 // [Dh]
    double* total = tbv + Dh;                 // [Dh]
    double* outmu = total + Dh;               // [nmax]
    double* scal = outmu + b.nmax;            // [0] largest emerging radiance of the order
    // ---- validity, air streams --------------------------------------------------------------------------------------
    int bad = 0;
    for (int l = 0; l < L; ++l) if (so_stage(b, SO_KIND, l, i) < 0.0) bad = 1;
    const cplx estar = bad ? cmk(1.0, 0.0) : so_estar(b, i, L);
    const double ria = csqrt_(estar).re;
    const int n_air = bad ? 0 : so_count_streams(b, ria);
    if (!bad) {
        for (int l = 0; l < L; ++l) if (b.nstream[i * b.Lmax + l] < 2) bad = 1;
        if (n_air < 1) bad = 1;
        // a Choudhury substrate out of its range under the last layer: the reference raises
        if (!substrate_in_range(b, s, frequency, cmk(so_stage(b, SO_EPS_RE, L - 1, i), so_stage(b, SO_EPS_IM, L - 1, i)))) bad = 1;
    }
    for (int it = 0; it < nt; ++it) { const double um = cos(b.theta[it]); if (!(um > 0.0 && um <= 1.0)) bad = 1; }
    if (bad) {
        for (int k = t; k < (NO + 1) * 2 * nt; k += NT) out[k] = NAN;
        for (int k = t; k < NO; k += NT) b.maxrad[i * NO + k] = NAN;
        for (int k = t; k <= b.nmax; k += NT) b.streams[i * (1 + b.nmax) + k] = 0.0;
        if (t == 0) { b.status[i] = ST_INPUT; b.orders[i] = 0; }
        return;
    }
    for (int j = t; j < n_air; j += NT) outmu[j] = so_mu(b, ria, j);
    for (int j = t; j < Dh; j += NT) total[j] = 0.0;
    for (int k = t; k <= b.nmax; k += NT) b.streams[i * (1 + b.nmax) + k] = k == 0 ? (double)n_air : (k <= n_air ? so_mu(b, ria, k - 1) : 0.0);
    // ---- workspace ----------------------------------------------------------------------------------------------------
    long long n_sub = 0;
    for (int l = 0; l < L; ++l) n_sub += b.nsub[i * b.Lmax + l];
    double* prof = b.ws + b.ws_off[i];                       // [n_sub + L][Dp]
    double* src = prof + (n_sub + L) * Dp;                   // [n_sub][Dp]
    double* bnd = src + n_sub * Dp;                          // [L][2][Dh]: reflections at the top (into the down sweep) / bottom (into the up sweep)
    const double* wt0 = b.wt + (i - b.chunk_begin) * b.Lmax * (long long)Dp * Dp;
    const double* vec0 = b.vec + i * b.Lmax * (long long)SO_VECS * Dh;
    const int lane = t & 63, wave = t >> 6;
    double tol = 0.0;
    int order = 0;
    block_sync();
    for (; order < NO; ++order) {
        if (order > 0) {
            // (a) the source of this order from the profile of the previous one
            long long itop = 0, isub = 0;
            for (int l = 0; l < L; ++l) {
                const int K = b.nsub[i * b.Lmax + l], n2 = 4 * b.nstream[i * b.Lmax + l], n16 = so_round16(n2);
                const double* wt = wt0 + l * (long long)Dp * Dp;
                for (int k0 = 0; k0 < K; k0 += 16) {
                    for (int idx = t; idx < 16 * n16; idx += NT) {
                        const int r = idx / n16, c = idx % n16, k = k0 + r;
                        double v = 0.0;
                        if (k < K && c < n2) v = (prof[(itop + k) * Dp + c] + prof[(itop + k + 1) * Dp + c]) / 2.0;
                        tile[r * LDm + c] = v;
                    }
                    block_sync();
                    for (int dt = wave; dt < n16 / 16; dt += NT / 64) {
                        tile4 acc = tile_zero();
                        for (int q0 = 0; q0 < n16; q0 += 4) {
                            const int q = q0 + (lane >> 4);
                            mfma_tile(tile[(lane & 15) * LDm + q], wt[(long long)q * Dp + dt * 16 + (lane & 15)], acc);
                        }
                        for (int reg = 0; reg < 4; ++reg) {
                            const int k = k0 + (lane >> 4) + 4 * reg;
                            if (k < K) src[(isub + k) * Dp + dt * 16 + (lane & 15)] = acc[reg];
                        }
                    }
                    block_sync();
                }
                // (b) specular reflection of the previous order at the two interfaces of the layer
                const int n = n2 / 2;
                const double* vec = vec0 + l * (long long)SO_VECS * Dh;
                for (int j = t; j < n; j += NT) {
                    bnd[(2 * l) * Dh + j] = vec[SO_RTOP * Dh + j] * prof[itop * Dp + j];
                    bnd[(2 * l + 1) * Dh + j] = vec[SO_RBOT * Dh + j] * prof[(itop + K) * Dp + n + j];
                }
                itop += K + 1; isub += K;
            }
            block_sync();
        }
        // (c) the two sweeps
        if (t < 128) {
            const int j = t;
            double carry = 0.0;
            long long itop = 0, isub = 0;
            for (int l = 0; l < L; ++l) {
                const int K = b.nsub[i * b.Lmax + l], n = 2 * b.nstream[i * b.Lmax + l];
                if (j < n) {
                    const double* vec = vec0 + l * (long long)SO_VECS * Dh;
                    const double e = vec[SO_EXT * Dh + j], ome = 1.0 - e;
                    const double s0 = b.srcterm[i * b.Lmax + l];
                    double I = (order > 0 ? bnd[(2 * l) * Dh + j] : 0.0) + carry;
                    prof[itop * Dp + n + j] = I;
                    for (int k = 0; k < K; ++k) {
                        const double sk = order > 0 ? src[(isub + k) * Dp + n + j] : s0;
                        I = I * e + sk * ome;
                        prof[(itop + k + 1) * Dp + n + j] = I;
                    }
                    carry = vec[SO_TBOT * Dh + j] * I;
                } else carry = 0.0;
                itop += K + 1; isub += K;
            }
        } else {
            const int j = t - 128;
            double carry = 0.0;
            long long itop = n_sub + L, isub = n_sub;
            for (int l = L - 1; l >= 0; --l) {
                const int K = b.nsub[i * b.Lmax + l], n = 2 * b.nstream[i * b.Lmax + l];
                itop -= K + 1; isub -= K;
                if (j < n) {
                    const double* vec = vec0 + l * (long long)SO_VECS * Dh;
                    const double e = vec[SO_EXT * Dh + j], ome = 1.0 - e;
                    const double s0 = b.srcterm[i * b.Lmax + l];
                    double I = (order > 0 ? bnd[(2 * l + 1) * Dh + j] : 0.0) + carry;
                    if (order == 0 && l == L - 1) I += vec[SO_EMIS * Dh + j];
                    prof[(itop + K) * Dp + j] = I;
                    for (int k = K - 1; k >= 0; --k) {
                        const double sk = order > 0 ? src[(isub + k) * Dp + j] : s0;
                        I = I * e + sk * ome;
                        prof[(itop + k) * Dp + j] = I;
                    }
                    carry = vec[SO_TTOP * Dh + j] * I;
                } else carry = 0.0;
            }
            if (j < 2 * n_air) emerg[j] = carry;   // (the air has no more streams than the first layer)
        }
        block_sync();
        // (d) the order's emerging radiance: stopping rule and brightness temperature
        if (t == 0) {
            double mx = emerg[0];
            for (int j = 1; j < 2 * n_air; ++j) mx = emerg[j] > mx ? emerg[j] : mx;
            scal[0] = mx;
            b.maxrad[i * NO + order] = mx;
        }
        for (int j = t; j < 2 * n_air; j += NT) {
            total[j] += emerg[j];
            tbv[j] = b.rj ? emerg[j] : planck_inverse(frequency, emerg[j]);
        }
        block_sync();
        for (int idx = t; idx < 2 * nt; idx += NT)
            out[(long long)order * 2 * nt + idx] = so_interpolate(outmu, tbv, n_air, idx / nt, cos(b.theta[idx % nt]));
        const double mx = scal[0];
        if (tol == 0.0) tol = b.rtol * mx;
        block_sync();   // (scal, tbv and emerg are rewritten by the next order)
        if (mx < tol) { ++order; break; }
    }
    for (int k = t + order * 2 * nt; k < NO * 2 * nt; k += NT) out[k] = 0.0;
    for (int k = t + order; k < NO; k += NT) b.maxrad[i * NO + k] = 0.0;
    for (int j = t; j < 2 * n_air; j += NT) tbv[j] = b.rj ? total[j] : planck_inverse(frequency, total[j]);
    block_sync();
    for (int idx = t; idx < 2 * nt; idx += NT)
        out[(long long)NO * 2 * nt + idx] = so_interpolate(outmu, tbv, n_air, idx / nt, cos(b.theta[idx % nt]));
    if (t == 0) { b.status[i] = ST_OK; b.orders[i] = order; }
}

}  // namespace smrt
