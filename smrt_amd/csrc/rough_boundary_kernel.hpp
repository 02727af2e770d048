// Rough boundaries evaluated on the device: geometrical_optics, geometrical_optics_backscatter and iem_fung92 as interfaces
// and as substrates (smrt_amd/interface/*.py, smrt_amd/substrate/*.py are the NumPy statements of the same models).  From the
// layer inputs of a batch the kernels write the buffers the dense composition reads -- host_interface, host_interface_coh,
// host_interface_slot, host_substrate, host_substrate_coh (include/smrt_dort.h) -- combined as DORT.interface_matrices /
// DORT.substrate_matrices combine them.  Four kernels, FP64:
//   rough_setup_block  one workgroup per pair: layer permittivities (layer_em, or host_layer), the most refringent layer,
//                      streams and weights of every layer and of the air (DORT._streams_of), the slot table
//   rough_go_block     geometrical_optics: one work item per (scattered stream, incident stream) of one of the four matrices,
//                      loop over the azimuth samples of [0, pi], cosine modes 0 .. m_max of the 2 x 2 V/H block in registers
//   rough_diag_block   iem_fung92 (Kirchhoff coherent part + backscatter series) and the lobe of
//                      geometrical_optics_backscatter: one work item per (matrix, stream), diagonal in the streams
//   rough_hemi_block   geometrical_optics_backscatter's coherent transmission, 1 - the hemispherical reflectivity of the full
//                      model: one workgroup per (boundary, direction, stream), 128 Gauss-Legendre cosines x 128 azimuths
// The block functions take the workgroup index; k_rough.hip wraps them in __global__ kernels, tests/hostemu/
// rough_boundary_host.cpp runs them under the fiber emulator.
#pragma once
#include "dort_layout.hpp"
#include "dort_physics.hpp"

namespace smrt {

enum { ROUGH_NONE = 0, ROUGH_GO = 1, ROUGH_GOB = 2, ROUGH_IEM = 3 };
constexpr int kRoughNT = 256;            // threads per workgroup of every kernel here
constexpr int kRoughHalf = 128;          // AZIMUTH_SAMPLES / 2: the modes are taken on kRoughHalf + 1 samples of [0, pi]
constexpr int kRoughQuad = 128;          // hemispherical reflectivity: Gauss-Legendre cosines and azimuth samples
constexpr int kRoughMMax = 4;            // largest m_max the mode accumulators are instantiated for (SMRT_ROUGH_M_MAX)
constexpr double kRoughMuFloor = 0.1;    // MU_FLOOR of geometrical_optics.py

struct RoughBatch {
    int S, Lmax, F, nmax;
    int nmodes;       // m_max + 1 in active mode, 1 in passive mode
    int active;
    int emmodel, micro;
    long long pair_begin, pair_count;
    const long long* pair_map;
    const int* n_layers;
    const double *frac_volume, *temperature, *p1, *p2, *frequency;
    const int* layer_kind;
    const double* liquid_water;
    const double* host_layer;
    const double* gl_mu;          // [nmax] the stream nodes in the most refringent layer
    const double* quad;           // [2][kRoughQuad] cosines on [0, 1] and weights of the 128-point Gauss-Legendre rule
    const int* rough_kind;        // [S][Lmax + 1]
    const double* rough_params;   // [S][Lmax + 1][4]
    const double *sub_p1, *sub_p2;   // [F][S] permittivity of a rough substrate
    int slots;        // rough interfaces per snowpack at most (host_interface_slots)
    int has_sub;      // the substrates of the batch are rough
    // per pair of the upload (index ip in 0 .. pair_count): streams of layer l at entry l, of the air at entry Lmax
    double *ws_mu, *ws_w;   // [pair_count][Lmax + 1][nmax]
    int* ws_n;              // [pair_count][Lmax + 1]; the air's count is 0 where the pair's inputs are invalid
    double* ws_eps;         // [pair_count][Lmax][2]
    // outputs, indexed by the global pair f * S + s like the arrays of the host route
    int* itf_slot;
    double *itf, *itf_coh, *sub, *sub_coh;
};

SMRT_DEV double rough_clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }   // (keeps a NaN, like np.clip)

// Smith's shadowing term of a Gaussian-slope surface (Tsang vol. III eq. 2.1.154)
SMRT_DEV double rough_shadowing(double s2, double cotangent) {
    const double v = cotangent / sqrt(2.0 * s2);
    return 0.5 * (exp(-v * v) / (sqrt(kPi) * v) - erfc(v));
}

// (h_out.k_in, v_out.k_in, h_in.k_out, v_in.k_out) / |k_in x k_out| with h_in = y; colinear directions: (-1, 0, 1, 0)
SMRT_DEV void rough_couplings(const double* ki, const double* ko, const double* ho, const double* vo, const double* vi, double* c) {
    const double a = ki[1] * ko[2] - ki[2] * ko[1], b = ki[2] * ko[0] - ki[0] * ko[2], d = ki[0] * ko[1] - ki[1] * ko[0];
    const double cross = sqrt(a * a + b * b + d * d);
    if (cross < 1e-4) { c[0] = -1.0; c[1] = 0.0; c[2] = 1.0; c[3] = 0.0; return; }
    c[0] = (ho[0] * ki[0] + ho[1] * ki[1] + ho[2] * ki[2]) / cross;
    c[1] = (vo[0] * ki[0] + vo[1] * ki[1] + vo[2] * ki[2]) / cross;
    c[2] = ko[1] / cross;
    c[3] = (vi[0] * ko[0] + vi[1] * ko[1] + vi[2] * ko[2]) / cross;
}

// One facet of the bistatic reflection (eqs. 2.1.122-124): o[2 ps + pi], the cosines already clipped to MU_FLOOR.
// shadow_den: 1 + the shadowing terms that count at this azimuth (1 without shadow correction)
SMRT_DEV void rough_go_reflection(cplx e1, cplx e2, double s2, double mu_s, double mu_i, double sin_s, double sin_i, double cp,
                                  double sp, double shadow_den, double* o) {
    const double ki[3] = {sin_i, 0.0, -mu_i}, ko[3] = {sin_s * cp, sin_s * sp, mu_s};
    const double q0 = ki[0] - ko[0], q1 = ki[1] - ko[1], q2_ = ki[2] - ko[2];
    const double qq = q0 * q0 + q1 * q1 + q2_ * q2_;
    const double sgn = (double)((q2_ > 0.0) - (q2_ < 0.0));
    const double mu_local = -(q0 * ki[0] + q1 * ki[1] + q2_ * ki[2]) / (sgn * sqrt(qq));
    cplx rv, rh; double mu2;
    fresnel_field(e1, e2, rough_clip(mu_local, kRoughMuFloor, 1.0), &rv, &rh, &mu2);
    const double ho[3] = {-sp, cp, 0.0}, vo[3] = {mu_s * cp, mu_s * sp, -sin_s}, vi[3] = {-mu_i, 0.0, -sin_i};
    double c[4];
    rough_couplings(ki, ko, ho, vo, vi, c);
    const double hh = c[0] * c[2], vv = c[1] * c[3], vh = c[1] * c[2], hv = c[0] * c[3];
    const double z2 = q2_ * q2_;
    const double factor = exp(-(q0 * q0 + q1 * q1) / (2.0 * z2 * s2)) / (4.0 * kPi * 2.0 * s2 * mu_i * z2 * z2) * (qq * qq) / shadow_den;
    o[0] = cabs2(cadd(cscale(rh, hh), cscale(rv, vv))) * factor;
    o[3] = cabs2(cadd(cscale(rh, vv), cscale(rv, hh))) * factor;
    o[2] = cabs2(csub(cscale(rh, vh), cscale(rv, hv))) * factor;
    o[1] = cabs2(csub(cscale(rh, hv), cscale(rv, vh))) * factor;
}

// One facet of the bistatic transmission from medium 1 into medium 2 (eqs. 2.1.128-132), real refractive indices in the
// geometry; `impossible` facets (no orientation refracts k_in into k_out) get r = -1.  ratio = n1 / n2, fre = Re(eps_2 / ratio).
SMRT_DEV void rough_go_transmission(double n1r, double n2r, cplx ratio, double fre, double s2, double mu_t, double mu_i, double sin_t,
                                    double sin_i, double cp, double sp, double shadow_den, double* o) {
    const double ki[3] = {sin_i, 0.0, -mu_i}, ko[3] = {sin_t * cp, sin_t * sp, -mu_t};
    const double q0 = ki[0] * n1r - ko[0] * n2r, q1 = ki[1] * n1r - ko[1] * n2r, q2_ = ki[2] * n1r - ko[2] * n2r;
    const double qq = q0 * q0 + q1 * q1 + q2_ * q2_;
    const double norm = (double)((q2_ > 0.0) - (q2_ < 0.0)) * sqrt(qq);
    const double n_kt = -(q0 * ko[0] + q1 * ko[1] + q2_ * ko[2]) / norm;
    const double n_ki = -(q0 * ki[0] + q1 * ki[1] + q2_ * ki[2]) / norm;
    double r_h = (n1r * n_ki - n2r * n_kt) / (n1r * n_ki + n2r * n_kt);
    double r_v = (n2r * n_ki - n1r * n_kt) / (n2r * n_ki + n1r * n_kt);
    if (n_kt < 0.0 || n_ki < 0.0) r_h = r_v = -1.0;
    const double ho[3] = {-sp, cp, 0.0}, vo[3] = {-mu_t * cp, -mu_t * sp, -sin_t}, vi[3] = {-mu_i, 0.0, -sin_i};
    double c[4];
    rough_couplings(ki, ko, ho, vo, vi, c);
    const double hh = c[0] * c[2], vv = c[1] * c[3], vh = c[1] * c[2], hv = c[0] * c[3];
    const double th = 1.0 + r_h;
    const cplx tv = cscale(ratio, 1.0 + r_v);
    const double z2 = q2_ * q2_;
    const double factor = fre * (2.0 * qq * n_kt * n_kt / (4.0 * kPi * s2 * mu_i * z2 * z2)) * exp(-(q0 * q0 + q1 * q1) / (2.0 * z2 * s2)) / shadow_den;
    o[0] = cabs2(cadd(cmk(hh * th, 0.0), cscale(tv, vv))) * factor;
    o[3] = cabs2(cadd(cmk(vv * th, 0.0), cscale(tv, hh))) * factor;
    o[2] = cabs2(cadd(cmk(-vh * th, 0.0), cscale(tv, hv))) * factor;
    o[1] = cabs2(csub(cmk(hv * th, 0.0), cscale(tv, vh))) * factor;
}

// iem_fung92's backscatter sigma0_pp / (4 pi mu), p = V, H (Fung et al. 1992 eqs. 82, 95): par = rms height, correlation
// length, autocorrelation id (0 exponential, 1 gaussian), series truncation
SMRT_DEV void rough_iem_backscatter(double frequency, cplx e1, cplx e2, double mu, const double* par, double* gamma) {
    const double rms = par[0], lc = par[1];
    const bool gaussian = par[2] != 0.0;
    const int terms = (int)par[3];
    const double k = 2.0 * kPi * frequency / kCSpeed * csqrt_(e1).re;
    const cplx eps_r = cdiv(e2, e1), one = cmk(1.0, 0.0);
    cplx rv, rh; double mu2;
    fresnel_field(e1, e2, mu, &rv, &rh, &mu2);
    const double sin2 = 1.0 - mu * mu, kz = k * mu, kx = k * sqrt(sin2), s2 = rms * rms;
    const cplx opv = cadd(one, rv), oph = cadd(one, rh);
    const cplx cv = cscale(cmul(cmul(cmul(opv, opv), csub(one, cdiv(one, eps_r))), cadd(one, cscale(cdiv(one, eps_r), sin2 / (mu * mu)))), sin2 / mu);
    const cplx ch = cscale(cmul(cmul(oph, oph), csub(eps_r, one)), sin2 / mu / (mu * mu));
    const cplx fv = cscale(rv, 2.0 / mu), fh = cscale(rh, -2.0 / mu);
    const double damp = exp(-s2 * kz * kz), q = -2.0 * kx;
    double p2kz = 1.0, pkz = 1.0, fact = 1.0, sum_v = 0.0, sum_h = 0.0;
    for (int n = 1; n <= terms; ++n) {
        p2kz *= 2.0 * kz; pkz *= kz; fact *= s2 / (double)n;
        const double x = q * lc / (double)n, y = 1.0 + x * x;
        const double spec = gaussian ? lc * lc / (2.0 * n) * exp(-((q * lc) * (q * lc)) / (4.0 * n))
                                     : (lc / n) * (lc / n) / (y * sqrt(y));   // (1 + x^2)^-1.5 without the library's pow
        const double weight = fact * spec, kir = p2kz * damp;
        sum_v += weight * cabs2(cadd(cscale(fv, kir), cscale(cv, pkz)));
        sum_h += weight * cabs2(csub(cscale(fh, kir), cscale(ch, pkz)));
    }
    const double front = k * k / 2.0 * exp(-2.0 * s2 * kz * kz);
    gamma[0] = front * sum_v / (4.0 * kPi * mu);
    gamma[1] = front * sum_h / (4.0 * kPi * mu);
}

// geometrical_optics_backscatter's lobe sigma0 / (4 pi mu), the same in V and H
SMRT_DEV double rough_gob_backscatter(cplx e1, cplx e2, double mu, double s2, bool shadow) {
    cplx rv, rh; double mu2;
    fresnel_field(e1, e2, 1.0, &rv, &rh, &mu2);
    const double tan2 = 1.0 / (mu * mu) - 1.0;
    double gamma = cabs2(rv) / (4.0 * kPi * 2.0 * s2 * (mu * mu * mu * mu * mu)) * exp(-tan2 / (2.0 * s2));
    if (shadow) gamma = gamma / (1.0 + rough_shadowing(s2, 1.0 / sqrt(tan2)));
    return gamma;
}

// Fresnel power diagonals (V, H, U) between lossy media and KirchhoffCoherentPart's attenuation (rms = 0: the flat surface)
SMRT_DEV void rough_kirchhoff_reflection(double frequency, cplx e1, cplx e2, double mu, double rms, double* r3) {
    cplx rv, rh; double mu2;
    fresnel_field(e1, e2, mu, &rv, &rh, &mu2);
    const double k0 = 2.0 * kPi * frequency / kCSpeed;
    const double k2 = k0 * k0 * cabs2(e1);   // (the reference scales the wavenumber by |eps_1|^2 here: kept)
    const double att = exp(-4.0 * k2 * rms * rms * mu * mu);
    r3[0] = cabs2(rv) * att; r3[1] = cabs2(rh) * att; r3[2] = cmul(rv, cconj(rh)).re * att;
}
SMRT_DEV void rough_kirchhoff_transmission(double frequency, cplx e1, cplx e2, double mu, double rms, double* t3) {
    cplx rv, rh; double mu2;
    fresnel_field(e1, e2, mu, &rv, &rh, &mu2);
    const double k0 = 2.0 * kPi * frequency / kCSpeed;
    const double kz_in = k0 * csqrt_(e1).re * mu;
    const double kz_out = k0 * csqrt_(csub(e2, cscale(e1, 1.0 - mu * mu))).re;
    const double d = (kz_out - kz_in) * rms, att = exp(-(d * d));
    const cplx one = cmk(1.0, 0.0);
    t3[0] = (1.0 - cabs2(rv)) * att; t3[1] = (1.0 - cabs2(rh)) * att;
    t3[2] = mu2 / mu * cmul(cadd(one, rv), cconj(cadd(one, rh))).re * att;
}

// ---- a boundary of a pair ---------------------------------------------------------------------------------------------
struct RoughTask {
    long long gp;
    int kind, k, sub;
    const double* par;
    double frequency;
    cplx e_low, e_up;                                 // interface: the layer and the medium above; substrate: last layer, substrate
    int n_low, n_up, n_t;
    const double *mu_low, *w_low, *mu_up, *w_up, *mu_t;
};

// task = ip * (slots + has_sub) + k: slot k of pair ip, or (k == slots) its substrate.  False: nothing to build.
SMRT_DEV bool rough_task(const RoughBatch& b, long long task, RoughTask* T) {
    const int nb = b.slots + b.has_sub;
    const long long ip = task / nb;
    const int k = (int)(task % nb);
    if (ip >= b.pair_count) return false;
    const long long gp = b.pair_map ? b.pair_map[b.pair_begin + ip] : b.pair_begin + ip;
    const int fi = (int)(gp / b.S), si = (int)(gp % b.S), L = b.n_layers[si], W = b.Lmax + 1;
    const int* n = b.ws_n + ip * W;
    if (n[b.Lmax] <= 0) return false;
    const int* kinds = b.rough_kind + (long long)si * W;
    const double* mu = b.ws_mu + ip * W * b.nmax;
    const double* w = b.ws_w + ip * W * b.nmax;
    const double* eps = b.ws_eps + ip * b.Lmax * 2;
    int li = -1;
    T->sub = (k == b.slots);
    if (T->sub) li = L;
    else
        for (int l = 0, c = 0; l < L; ++l)
            if (kinds[l] != ROUGH_NONE && c++ == k) { li = l; break; }
    if (li < 0 || kinds[li] == ROUGH_NONE) return false;
    T->gp = gp; T->k = k; T->kind = kinds[li]; T->par = b.rough_params + ((long long)si * W + li) * 4;
    T->frequency = b.frequency[fi];
    // the entries of the workspace the boundary reads.  One set of stores for both cases: with the stores inside the branches
    // the compiler merges them into stores through a choice of fields, which keeps the task in scratch (24 bytes per lane)
    int low, up, tr;
    if (T->sub) {
        low = up = tr = L - 1;
        T->e_up = cmk(b.sub_p1[(long long)fi * b.S + si], b.sub_p2[(long long)fi * b.S + si]);
    } else {
        low = li; up = li > 0 ? li - 1 : b.Lmax;
        tr = li > 1 ? li - 1 : b.Lmax;   // (the cosines of the upward diffuse transmission: the reference's choice)
        T->e_up = li > 0 ? cmk(eps[2 * up], eps[2 * up + 1]) : cmk(1.0, 0.0);
    }
    T->e_low = cmk(eps[2 * low], eps[2 * low + 1]);
    T->n_low = n[low]; T->n_up = n[up]; T->n_t = n[tr];
    T->mu_low = mu + (long long)low * b.nmax; T->w_low = w + (long long)low * b.nmax;
    T->mu_up = mu + (long long)up * b.nmax; T->w_up = w + (long long)up * b.nmax;
    T->mu_t = mu + (long long)tr * b.nmax;
    return true;
}

// where matrix q of mode m of the task lies (leading dimension NE = 3 nmax), and its specular diagonal
SMRT_DEV double* rough_matrix(const RoughBatch& b, const RoughTask& T, int m, int q) {
    const long long ne2 = 9LL * b.nmax * b.nmax;
    if (T.sub) return b.sub + (T.gp * b.nmodes + m) * ne2;
    return b.itf + (((T.gp * b.slots + T.k) * b.nmodes + m) * 4 + q) * ne2;
}
SMRT_DEV double* rough_coh(const RoughBatch& b, const RoughTask& T, int m, int q) {
    if (T.sub) return b.sub_coh + (T.gp * b.nmodes + m) * 3LL * b.nmax;
    return b.itf_coh + ((T.gp * b.slots + T.k) * 4 + q) * 3LL * b.nmax;
}

// ---- setup: permittivities, streams, slot table -------------------------------------------------------------------------
SMRT_DEV cplx rough_layer_eps(const RoughBatch& b, long long gp, int si, int l, double frequency, int* bad) {
    const long long o = (long long)si * b.Lmax + l;
    const int kind = b.layer_kind ? b.layer_kind[o] : b.emmodel + 16 * b.micro;
    const int em = kind & 15;
    if (em == EM_HOST || em == EM_IBA_HOST || em == EM_RAYLEIGH_HOST) {   // where the batch carries host_layer: from there
        if (!b.host_layer) { *bad = 1; return cmk(1.0, 0.0); }
        const double* h = b.host_layer + (gp * b.Lmax + l) * 4;
        if (!(h[1] >= 0.0) || !(h[2] > 0.0)) *bad = 1;
        return cmk(h[2], h[3]);
    }
    cplx ee; double ks, ka, pa, pb;
    layer_em(em, kind >> 4, frequency, b.frac_volume[o], b.temperature[o], b.p1[o], b.p2[o], &ee, &ks, &ka, &pa, &pb, bad,
             b.liquid_water ? b.liquid_water[o] : 0.0);
    if (!(ks >= 0.0)) *bad = 1;
    return ee;
}

SMRT_DEV void rough_setup_block(const RoughBatch& b, long long ip, int* flags /* LDS: [2] */) {
    const int t = tid(), W = b.Lmax + 1, nmax = b.nmax;
    const long long gp = b.pair_map ? b.pair_map[b.pair_begin + ip] : b.pair_begin + ip;
    const int fi = (int)(gp / b.S), si = (int)(gp % b.S), L = b.n_layers[si];
    const double frequency = b.frequency[fi];
    double* eps = b.ws_eps + ip * b.Lmax * 2;
    int* n = b.ws_n + ip * W;
    if (t < 2) flags[t] = 0;
    block_sync();
    for (int l = t; l < L; l += kRoughNT) {
        int bad = 0;
        const cplx ee = rough_layer_eps(b, gp, si, l, frequency, &bad);
        eps[2 * l] = ee.re; eps[2 * l + 1] = ee.im;
        if (bad) lds_max(&flags[0], 1);
    }
    block_sync();
    if (t == 0) {   // the most refringent layer: first maximum of (Re, Im)
        int star = 0;
        for (int l = 1; l < L; ++l)
            if (eps[2 * l] > eps[2 * star] || (eps[2 * l] == eps[2 * star] && eps[2 * l + 1] > eps[2 * star + 1])) star = l;
        flags[1] = star;
        // the slot table: the k-th rough interface of the snowpack takes slot k
        const int* kinds = b.rough_kind + (long long)si * W;
        for (int l = 0, c = 0; l < b.Lmax && b.slots > 0; ++l)
            b.itf_slot[gp * b.Lmax + l] = (l < L && kinds[l] != ROUGH_NONE) ? c++ : -1;
    }
    block_sync();
    const cplx estar = cmk(eps[2 * flags[1]], eps[2 * flags[1] + 1]);
    for (int l = t; l <= L; l += kRoughNT) {
        const int e = l < L ? l : b.Lmax;   // the air after the layers
        const cplx el = l < L ? cmk(eps[2 * l], eps[2 * l + 1]) : cmk(1.0, 0.0);
        const double ri = csqrt_(cdiv(estar, el)).re;
        double* mu = b.ws_mu + (ip * W + e) * nmax;
        double* w = b.ws_w + (ip * W + e) * nmax;
        int c = 0;
        for (int j = 0; j < nmax; ++j) {
            const double g = b.gl_mu[j], rs = ri * sqrt(1.0 - g * g);
            if (rs < 1.0) mu[c++] = sqrt(1.0 - rs * rs);
        }
        if (c < (l < L ? 2 : 1)) { lds_max(&flags[0], 1); c = 0; }   // (what the solve refuses as well)
        if (c == 1) w[0] = NAN;   // a single air stream has no weight (the reference's weights need two): a rough surface on it is NaN
        for (int j = 0; j < c && c > 1; ++j) {
            const double v = j == 0 ? 1.0 - 0.5 * (mu[0] + mu[1]) : j == c - 1 ? 0.5 * (mu[c - 2] + mu[c - 1]) : 0.5 * (mu[j - 1] - mu[j + 1]);
            w[j] = l < L ? fabs(v) : v;   // absolute for the layers, signed for the air
        }
        n[e] = c;
    }
    block_sync();
    if (t == 0 && flags[0]) n[b.Lmax] = 0;   // invalid inputs: nothing is built, the solve reports the pair
}

// ---- geometrical_optics ------------------------------------------------------------------------------------------------------
// LDS: cos / sin of the kRoughHalf + 1 azimuths, then MM rows of mode weights (end-point weight x cos(m phi) x norm)
constexpr int kRoughGoLds = (2 + kRoughMMax + 1) * (kRoughHalf + 1);

template <int MM>
SMRT_DEV void rough_go_block(const RoughBatch& b, long long blk, double* lds) {
    constexpr int NPH = kRoughHalf + 1;
    const int t = tid(), nmax = b.nmax;
    const int tiles = (nmax * nmax + kRoughNT - 1) / kRoughNT;
    const int tile = (int)(blk % tiles), q = (int)((blk / tiles) % 4);
    RoughTask T;
    if (!rough_task(b, blk / (4LL * tiles), &T) || T.kind != ROUGH_GO || (T.sub && q != 0)) return;   // (uniform over the workgroup)
    double *cphi = lds, *sphi = lds + NPH, *wm = lds + 2 * NPH;
    for (int k = t; k < NPH; k += kRoughNT) {
        const double ph = k == kRoughHalf ? kPi : (double)k * (kPi / kRoughHalf);
        cphi[k] = cos(ph); sphi[k] = sin(ph);
        const double end = (k == 0 || k == kRoughHalf) ? 1.0 : 2.0;
        for (int m = 0; m < MM; ++m) wm[m * NPH + k] = end * cos((double)m * ph) * ((m == 0 ? 1.0 : 2.0) / (2 * kRoughHalf));
    }
    block_sync();
    const int idx = tile * kRoughNT + t;
    const int s = idx / nmax, i = idx % nmax;
    const bool trans = (q & 1) != 0;
    // scattered / incident streams, media and the rows that exist (interface_matrices.combined, _interfaces_on_host)
    const double* mus = q == 0 ? T.mu_low : q == 1 ? T.mu_t : q == 2 ? T.mu_up : T.mu_low;
    const double* mui = (q == 0 || q == 1) ? T.mu_low : T.mu_up;
    const double* wi = (q == 0 || q == 1) ? T.w_low : T.w_up;
    const int n_i = (q == 0 || q == 1) ? T.n_low : T.n_up;
    const int rows = q == 0 ? T.n_low : q == 1 ? (T.n_t < T.n_up ? T.n_t : T.n_up) : q == 2 ? T.n_up : T.n_low;
    if (idx >= nmax * nmax || s >= rows || i >= n_i) return;
    const cplx e1 = (q == 0 || q == 1) ? T.e_low : T.e_up, e2 = (q == 0 || q == 1) ? T.e_up : T.e_low;
    const double s2 = T.par[0];
    const bool shadow = T.par[1] != 0.0;
    const double mu_s = rough_clip(mus[s], kRoughMuFloor, 1.0), mu_i = rough_clip(mui[i], kRoughMuFloor, 1.0);
    const double sin_s = sqrt(1.0 - mu_s * mu_s), sin_i = sqrt(1.0 - mu_i * mu_i);
    double lam_i = 0.0, lam_s = 0.0;
    if (shadow) {
        lam_i = rough_shadowing(s2, mu_i / (sin_i > 1e-3 ? sin_i : 1e-3));
        lam_s = rough_shadowing(s2, mu_s / (sin_s > 1e-3 ? sin_s : 1e-3));
    }
    const double den = 1.0 + lam_i + lam_s;
    // in the backscattering half-plane (phi == pi exactly: the last sample) the lower direction is already counted
    const double den_back = trans ? den : (mu_s <= mu_i ? 1.0 + lam_s : 1.0 + lam_i);
    const cplx n1 = csqrt_(e1), n2 = csqrt_(e2), ratio = cdiv(n1, n2);
    double fre = cdiv(e2, ratio).re;
    if (trans && sqrt(cabs2(csub(ratio, cmk(1.0, 0.0)))) < 1e-6) fre = NAN;   // identical indices: not implemented in the model
    double acc[MM][4];
#pragma unroll
    for (int m = 0; m < MM; ++m) acc[m][0] = acc[m][1] = acc[m][2] = acc[m][3] = 0.0;
    for (int k = 0; k < NPH; ++k) {
        double o[4];
        const double dk = k == kRoughHalf ? den_back : den;
        if (trans) rough_go_transmission(n1.re, n2.re, ratio, fre, s2, mu_s, mu_i, sin_s, sin_i, cphi[k], sphi[k], dk, o);
        else rough_go_reflection(e1, e2, s2, mu_s, mu_i, sin_s, sin_i, cphi[k], sphi[k], dk, o);
#pragma unroll
        for (int m = 0; m < MM; ++m) {
            const double wk = wm[m * NPH + k];
            acc[m][0] += wk * o[0]; acc[m][1] += wk * o[1]; acc[m][2] += wk * o[2]; acc[m][3] += wk * o[3];
        }
    }
    // column x mu_i w_i, row / mu_s, the ratio of the real permittivities on the transmissions, 2 pi | pi
    const double scale = trans ? e1.re / e2.re : 1.0;
    const double colrow = (mui[i] * wi[i]) / mus[s];
    const long long NE = 3LL * nmax;
#pragma unroll
    for (int m = 0; m < MM; ++m) {
        const int P = m == 0 ? 2 : 3;
        const double coef = m == 0 ? 2.0 * kPi : kPi;
        double* M = rough_matrix(b, T, m, q);
        for (int ps = 0; ps < 2; ++ps)
            for (int pi = 0; pi < 2; ++pi)
                M[(long long)(s * P + ps) * NE + i * P + pi] = coef * (acc[m][2 * ps + pi] * scale * colrow);
    }
}

// ---- iem_fung92 and the lobe of geometrical_optics_backscatter: diagonal in the streams --------------------------------------
SMRT_DEV void rough_diag_block(const RoughBatch& b, long long blk) {
    const int nmax = b.nmax;
    const long long item = blk * kRoughNT + tid();
    const int j = (int)(item % nmax), q = (int)((item / nmax) % 4);
    RoughTask T;
    if (!rough_task(b, item / (4LL * nmax), &T) || T.kind == ROUGH_GO || (T.sub && q != 0)) return;
    const bool iem = T.kind == ROUGH_IEM, low = (q == 0 || q == 1), trans = (q & 1) != 0;
    const int n1 = low ? T.n_low : T.n_up, n2 = low ? T.n_up : T.n_low;
    if (j >= n1) return;
    const cplx e1 = low ? T.e_low : T.e_up, e2 = low ? T.e_up : T.e_low;
    const double mu = (low ? T.mu_low : T.mu_up)[j], w = (low ? T.w_low : T.w_up)[j];
    const double f = T.frequency;
    const long long NE = 3LL * nmax;
    const int m_max = b.nmodes - 1;
    if (trans) {   // coherent transmission, cut to the common streams; geometrical_optics_backscatter's: rough_hemi_block
        if (!iem) return;
        double t3[3];
        rough_kirchhoff_transmission(f, e1, e2, mu, T.par[0], t3);
        if (j < n2) {
            for (int m = 0; m < b.nmodes; ++m) {
                const int P = m == 0 ? 2 : 3;
                double* M = rough_matrix(b, T, m, q);
                for (int p = 0; p < P; ++p) M[(long long)(j * P + p) * NE + j * P + p] = t3[p];
            }
            double* c = rough_coh(b, T, 0, q);
            c[2 * j] = t3[0]; c[2 * j + 1] = t3[1];
        }
        return;
    }
    double r3[3] = {0.0, 0.0, 0.0}, gamma[2];
    if (iem) {
        rough_kirchhoff_reflection(f, e1, e2, mu, T.par[0], r3);
        rough_iem_backscatter(f, e1, e2, mu, T.par, gamma);
    } else gamma[0] = gamma[1] = rough_gob_backscatter(e1, e2, mu, T.par[0], T.par[1] != 0.0);
    for (int m = 0; m < b.nmodes; ++m) {   // the lobe spread over the modes: 1, -2, +2, ... / (1 + 2 m_max)
        const int P = m == 0 ? 2 : 3;
        const double coef = m == 0 ? 2.0 * kPi : kPi;
        const double cm = (m == 0 ? 1.0 : ((m & 1) ? -2.0 : 2.0)) / (double)(1 + 2 * m_max);
        double* M = rough_matrix(b, T, m, q);
        for (int p = 0; p < P; ++p)
            M[(long long)(j * P + p) * NE + j * P + p] = r3[p] + (p < 2 ? coef * (cm * gamma[p] * w) : 0.0);
        if (T.sub) {   // the substrate keeps the specular diagonal of every mode, in the mode's own compressed order
            double* c = rough_coh(b, T, m, 0);
            for (int p = 0; p < P; ++p) c[j * P + p] = r3[p];
        }
    }
    if (!T.sub) {
        double* c = rough_coh(b, T, 0, q);
        c[2 * j] = r3[0]; c[2 * j + 1] = r3[1];
    } else if (!b.active) {   // passive mode: the emissivity takes the place of the specular diagonal
        double t3[3] = {0.0, 0.0, 0.0};
        if (iem) rough_kirchhoff_transmission(f, e1, e2, mu, T.par[0], t3);
        double* c = rough_coh(b, T, 0, 0);
        if (iem) { c[2 * j] = t3[0]; c[2 * j + 1] = t3[1]; }
    }
}

// ---- geometrical_optics_backscatter: coherent transmission = 1 - hemispherical reflectivity of the full model ------------------
// one workgroup per (task, direction, stream); thread t: cosine t % 128, azimuths 64 (t / 128) .. + 64; shadow correction on,
// whatever the object says (the finding recorded in geometrical_optics_backscatter.py).  LDS: [2][128] azimuth table + [2][256]
constexpr int kRoughHemiLds = 2 * kRoughQuad + 2 * kRoughNT;

SMRT_DEV void rough_hemi_block(const RoughBatch& b, long long blk, double* lds) {
    const int t = tid(), nmax = b.nmax;
    const int j = (int)(blk % nmax), dir = (int)((blk / nmax) % 2);
    RoughTask T;
    if (!rough_task(b, blk / (2LL * nmax), &T) || T.kind != ROUGH_GOB) return;
    if (T.sub && (dir != 0 || b.active)) return;   // a substrate emits through it in passive mode only
    const bool low = dir == 0;
    const int n1 = low ? T.n_low : T.n_up, n2 = low ? T.n_up : T.n_low;
    if (j >= n1) return;
    double *cphi = lds, *sphi = lds + kRoughQuad, *red = lds + 2 * kRoughQuad;
    for (int k = t; k < kRoughQuad; k += kRoughNT) {
        const double ph = (double)k * (2.0 * kPi / kRoughQuad);
        cphi[k] = cos(ph); sphi[k] = sin(ph);
    }
    block_sync();
    const cplx e1 = low ? T.e_low : T.e_up, e2 = low ? T.e_up : T.e_low;
    const double s2 = T.par[0];
    const double mu_i = rough_clip((low ? T.mu_low : T.mu_up)[j], kRoughMuFloor, 1.0);
    const int a = t % kRoughQuad, half = t / kRoughQuad;
    const double mu_s = rough_clip(b.quad[a], kRoughMuFloor, 1.0), wa = b.quad[kRoughQuad + a];
    const double sin_s = sqrt(1.0 - mu_s * mu_s), sin_i = sqrt(1.0 - mu_i * mu_i);
    const double lam_i = rough_shadowing(s2, mu_i / (sin_i > 1e-3 ? sin_i : 1e-3));
    const double lam_s = rough_shadowing(s2, mu_s / (sin_s > 1e-3 ? sin_s : 1e-3));
    const double den = 1.0 + lam_i + lam_s, den_back = mu_s <= mu_i ? 1.0 + lam_s : 1.0 + lam_i;
    double sv = 0.0, sh = 0.0;
    for (int k = half * (kRoughQuad / 2); k < (half + 1) * (kRoughQuad / 2); ++k) {
        double o[4];
        rough_go_reflection(e1, e2, s2, mu_s, mu_i, sin_s, sin_i, cphi[k], sphi[k], k == kRoughQuad / 2 ? den_back : den, o);
        sv += o[0] + o[2]; sh += o[1] + o[3];   // summed over the scattered polarisation
    }
    red[t] = wa * sv; red[kRoughNT + t] = wa * sh;
    block_sync();
    for (int step = kRoughNT / 2; step >= 1; step >>= 1) {
        if (t < step) { red[t] += red[t + step]; red[kRoughNT + t] += red[kRoughNT + t + step]; }
        block_sync();
    }
    if (t != 0) return;
    const double tv = 1.0 - 2.0 * kPi / kRoughQuad * red[0], th = 1.0 - 2.0 * kPi / kRoughQuad * red[kRoughNT];
    if (T.sub) {
        double* c = rough_coh(b, T, 0, 0);
        c[2 * j] = tv; c[2 * j + 1] = th;
        return;
    }
    const int q = low ? 1 : 3;
    const long long NE = 3LL * nmax;
    if (j < n2) {
        for (int m = 0; m < b.nmodes; ++m) {
            const int P = m == 0 ? 2 : 3;
            double* M = rough_matrix(b, T, m, q);
            M[(long long)(j * P) * NE + j * P] = tv; M[(long long)(j * P + 1) * NE + j * P + 1] = th;
        }
        double* c = rough_coh(b, T, 0, q);
        c[2 * j] = tv; c[2 * j + 1] = th;
    }
}

}  // namespace smrt
