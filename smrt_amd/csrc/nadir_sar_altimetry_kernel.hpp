// Nadir SAR altimetry solver (the reference's smrt/rtsolver/nadir_sar_altimetry.py with the delay-Doppler model of
// delay_doppler_model/dinardo18.py: Dinardo et al. 2018, Ray et al. 2015): the arithmetic of its kernels.
//
//   lrm_layer_item, lrm_vertical_pair   of nadir_lrm_altimetry_kernel.hpp with LrmBatch.sar set: the layer scalars and the
//                       volume backscatter per sub-gate (one row, no echo in it).
//   sar_boundary_pair   same workgroup as the vertical distribution: the coherent and incoherent echo of every boundary
//                       attenuated down to it, its two-way travel time and its shift in samples.
//   sar_table_item      one (table, delay, Doppler) sample of f0(tau / sigma_c) and f1(tau / sigma_c) (D18 eq. 9-12): one pair of
//                       tables per distinct sigma_surface of the group.
//   sar_combine_item    one workgroup per (pair, coarse Doppler bin): the fine columns of the base map (D18 eq. 22, nu = 0) in
//                       LDS, the direct convolution with the volume backscatter, the shifted and scaled columns of the
//                       boundaries at their own nu, the row map, the mean over the oversampling blocks.
// With the model of Halimi et al. 2014 (delay_doppler_model/halimi14.py) the table stage is sar_h14_doppler_row,
// sar_h14_kernel_table and sar_h14_delay_column instead, and sar_combine_model<kSarHalimi14> reads the one table of the pair.
//
// With -DSMRT_HOST_EMU (g++, the CPU tests) a workgroup is one thread.
#pragma once
#include "nadir_lrm_altimetry_kernel.hpp"

namespace smrt {

constexpr int kSarThreads = 256;
constexpr double kSarCrossover = 30.0;   // x = xi^2 / 4 below: ascending series; at and above: Hankel's asymptotic expansion
// doubles per (snowpack, boundary) of smrt_sar_params.boundary_values and per (pair, boundary) of the echo output
enum { SAR_BV_TRANS = 0, SAR_BV_COHERENT, SAR_BV_INCOHERENT, SAR_BV_NU, SAR_BV };
enum { SAR_ECHO_TIME = 0, SAR_ECHO_COHERENT, SAR_ECHO_INCOHERENT, SAR_ECHO_SHIFT, SAR_ECHO };

struct SarBatch {
    LrmBatch lrm;                    // rows = 1, n_mu = 1, sar = 1, itf = boundary_values; lrm.out is not used
    int ndoppler, osd, ND;           // ND = ndoppler * osd
    int out_rows, n_tab, n_t, n_d;   // samples of an output row: n_t x n_d
    double prf, wavelength, velocity, alpha, pitch, roll, sigma_p, theta_lim, gamma_x, gamma_y, l_gamma, lz, pu, nu_coherent;
    const double* tab_sigma;         // [n_tab] sigma_surface of every table
    const int* tab_index;            // [S]
    const int* row_map;              // [S][2 (Lmax + 1) + 2]: incoherent boundaries, coherent boundaries, volume -> output row or -1;
                                     // then the row of the total (every source), or -1
    double* tables;                  // [n_tab][2][N][ND]
    double* echo;                    // [n_pairs][Lmax + 1][SAR_ECHO]
    double* out;                     // [n_pairs][out_rows][n_t][n_d]
    // Halimi et al. 2014 (model == kSarHalimi14; all zero with Dinardo18): `tables` is then [n_tab][ND][N], ONE table per
    // sigma_surface, delay fastest
    int model, slant, N_wide, M;     // N_wide = N x delay_window_widening; M = 2 (N / 2) - 1 samples of the delay kernel
    double h14_pu, h14_gamma, idelta_r1;
    double* h14_doppler;             // [ND][N_wide] the impulse response convolved along Doppler, delay fastest
    double* h14_kernel;              // [n_tab][M] sinc^2 convolved with the height distribution
};
enum { kSarDinardo18 = 0, kSarHalimi14 = 1 };

// ---- I_v(x) e^-x for v = -3/4, -1/4, 1/4, 3/4 and x >= 0 ---------------------------------------------------------------------
// which: 0 .. 3 in that order.  The ascending series has positive terms only; the asymptotic expansion depends on v^2.
SMRT_DEV double sar_ive(int which, double x) {
    const double v = which == 0 ? -0.75 : which == 1 ? -0.25 : which == 2 ? 0.25 : 0.75;
    if (x < kSarCrossover) {
        // Gamma(v + 1): Gamma(1/4), Gamma(3/4), Gamma(5/4), Gamma(7/4)
        const double g = which == 0 ? 3.625609908221908 : which == 1 ? 1.2254167024651776 : which == 2 ? 0.9064024770554771 : 0.9190625268488832;
        const double q = 0.25 * x * x;
        double term = 1.0, sum = 1.0;
        for (int k = 1; k < 300; ++k) {
            term *= q / ((double)k * ((double)k + v));
            sum += term;
            if (term < 1e-17 * sum) break;
        }
        return pow(0.5 * x, v) / g * sum * exp(-x);
    }
    const double mu = 4.0 * v * v;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 60; ++k) {
        const double odd = 2.0 * k - 1.0;
        term *= -(mu - odd * odd) / (8.0 * x * k);
        if (fabs(term) < 1e-17) break;
        sum += term;
    }
    return sum / sqrt(2.0 * kPi * x);
}

SMRT_DEV double sar_sign(double x) { return x > 0.0 ? 1.0 : x < 0.0 ? -1.0 : 0.0; }

SMRT_DEV double sar_f0(double xi) {   // D18 eq. 9, eq. 11 at the origin
    const double x = xi * xi / 4.0;
    if (x < 1e-20) return kPi * 1.681792830507429 / (4.0 * 1.2254167024651776);
    return kPi / 4.0 * sqrt(fabs(xi)) * (sar_ive(1, x) + sar_sign(xi) * sar_ive(2, x));
}

SMRT_DEV double sar_f1(double xi) {   // D18 eq. 10, eq. 12 at the origin
    const double x = xi * xi / 4.0;
    if (x < 1e-20) return -1.681792830507429 * 1.2254167024651776 / 4.0;
    const double a = fabs(xi);
    return kPi / 8.0 * (a * sqrt(a)) * ((sar_ive(2, x) - sar_ive(0, x)) + sar_sign(xi) * (sar_ive(1, x) - sar_ive(3, x)));
}

// ---- the axes ---------------------------------------------------------------------------------------------------------------
SMRT_DEV double sar_tau(const SarBatch& b, int n) { return ((double)n / b.lrm.os - b.lrm.nominal_gate) / b.lrm.bandwidth; }
SMRT_DEV double sar_look_angle(const SarBatch& b, int c) {
    const double fd = (-(double)(b.ndoppler / 2 * b.osd) + 0.5 + c) * (b.prf / ((double)b.osd * b.ndoppler));
    return b.wavelength / (2.0 * b.velocity) * fd;
}
SMRT_DEV double sar_sigma_c(const SarBatch& b, double look, double sigma_surface) {
    const double r = look / b.theta_lim, s = 2.0 * sigma_surface / kCSpeed;
    return sqrt(b.sigma_p * b.sigma_p * (1.0 + r * r) + s * s);
}
SMRT_DEV double sar_f(const SarBatch& b, int n) {   // D18 eq. 25
    const double f = kCSpeed / (b.alpha * b.lrm.altitude) * sar_tau(b, n);
    return f > 0.0 ? f : 0.0;
}

// ---- the echo of the boundaries of one pair (after lrm_vertical_pair, same workgroup) ---------------------------------------
SMRT_DEV void sar_boundary_pair(const SarBatch& b, long long i, int tid, int nt) {
    const LrmBatch& lb = b.lrm;
    const long long gp = lrm_global_pair(lb, i);
    const int s = (int)(gp % lb.fo.S);
    const int L = lb.fo.n_layers[s], Lmax = lb.fo.Lmax;
    double* e = b.echo + i * (Lmax + 1) * SAR_ECHO;
    // (every lane reads the status of the vertical distribution before any lane marks the pair below)
    const int status = lb.status[i];
    lrm_sync();
    if (status != ST_OK) {
        for (int k = tid; k < (Lmax + 1) * SAR_ECHO; k += nt) e[k] = NAN;
        return;
    }
    const double* pre = lb.prefix + i * LRM_PREFIX_ROWS * (Lmax + 1);
    const double* bv = lb.itf + gp * (Lmax + 1) * SAR_BV;
    const double step = lb.bandwidth * lb.os;
    for (int k = tid; k <= Lmax; k += nt) {
        double* ek = e + k * SAR_ECHO;
        if (k > L) { ek[0] = ek[1] = ek[2] = ek[3] = 0.0; continue; }
        double tau = 0.0;
        for (int l = 0; l < k; ++l) tau += 2.0 * (fo_stage(lb.fo, FO_KS, l, i) + fo_stage(lb.fo, FO_KA, l, i)) * fo_stage(lb.fo, FO_THICK, l, i);
        const double att = exp(-tau) * pre[LRM_CUMTRANS * (Lmax + 1) + k];
        const double t = pre[LRM_TLAY * (Lmax + 1) + k];
        const double coh = bv[k * SAR_BV + SAR_BV_COHERENT] * att, inc = bv[k * SAR_BV + SAR_BV_INCOHERENT] * att;
        const double shift = rint(t * step);   // half to even, as numpy.round
        ek[SAR_ECHO_TIME] = t; ek[SAR_ECHO_COHERENT] = coh; ek[SAR_ECHO_INCOHERENT] = inc; ek[SAR_ECHO_SHIFT] = shift;
        // the reference's `assert 0 <= itime < N`; a NaN echo is an input error as well
        const bool outside = !(shift >= 0.0 && shift < (double)lb.N);
        if (coh != coh || inc != inc || ((coh > 0.0 || inc > 0.0) && outside)) lb.status[i] = ST_INPUT;
    }
}

// ---- the tables -------------------------------------------------------------------------------------------------------------
SMRT_DEV void sar_table_item(const SarBatch& b, long long idx) {
    const int N = b.lrm.N, ND = b.ND;
    const int c = (int)(idx % ND), n = (int)((idx / ND) % N), t = (int)(idx / ((long long)ND * N));
    const double xi = sar_tau(b, n) / sar_sigma_c(b, sar_look_angle(b, c), b.tab_sigma[t]);
    double* tab = b.tables + (size_t)t * 2 * N * ND;
    tab[(size_t)n * ND + c] = sar_f0(xi);
    tab[(size_t)N * ND + (size_t)n * ND + c] = sar_f1(xi);
}

// ---- the table of Halimi et al. 2014 (delay_doppler_model/halimi14.py, delay_doppler_utils.py) ---------------------------------
// The flat-surface impulse response (H14 eq. 11-14) is closed form; the point target responses and the height distribution
// enter through three linear convolutions ("same" alignment of scipy.signal.fftconvolve), made here by direct summation:
// a thread owns consecutive outputs, so the sliding operand is read conflict-free and the other one as a broadcast.
inline size_t sar_h14_doppler_lds_bytes(int ND) { return (size_t)3 * ND * sizeof(double); }            // phi, impulse response, sinc^2
inline size_t sar_h14_kernel_lds_bytes(int M) { return (size_t)2 * M * sizeof(double); }                // sinc^2, Gaussian
inline size_t sar_h14_delay_lds_bytes(int N_wide, int M) { return ((size_t)N_wide + M) * sizeof(double); }   // column, delay kernel
inline size_t sar_h14_combine_lds_bytes(int N, int osd) { return (size_t)N * (1 + 3 * (size_t)osd) * sizeof(double); }

// What the host derives of smrt_sar_params for Halimi14, once the sensor and the shape are in `d` (the device launch and the CPU
// build alike): the shapes, and idelta_r1 of delay_doppler_utils.py:_compute_idelta_r1 (H14 eq. 19 in samples, with the Earth's curvature).
inline void sar_h14_setup(SarBatch& d, int slant, int widening, double h14_pu, double h14_gamma, double burst_duration) {
    d.model = kSarHalimi14; d.slant = slant; d.N_wide = d.lrm.N * widening; d.M = 2 * (d.lrm.N / 2) - 1;
    d.h14_pu = h14_pu; d.h14_gamma = h14_gamma;
    const double f1 = 1.0 / burst_duration / d.osd;
    const double delta_r1 = f1 * f1 * (d.alpha * d.lrm.altitude * (d.wavelength * d.wavelength) / (8.0 * (d.velocity * d.velocity)));
    d.idelta_r1 = delta_r1 * (2.0 / kCSpeed * d.lrm.bandwidth * d.lrm.os);
}

SMRT_DEV double sar_sinc2(double x) {   // numpy.sinc(x)^2
    if (x == 0.0) return 1.0;
    const double s = sin(kPi * x) / (kPi * x);
    return s * s;
}

SMRT_DEV double sar_doppler_frequency(const SarBatch& b, int c) {
    return (-(double)(b.ndoppler / 2 * b.osd) + 0.5 + c) * (b.prf / ((double)b.osd * b.ndoppler));
}

// One workgroup per delay n of the widened window: phi (eq. 12; NaN outside the circle), its difference along Doppler as
// halimi14.py:diff_cyclic takes it -- the LAST column is phi[0] - phi[1], not a cyclic difference, and negative --, NaN -> 0, the
// convolution with the Doppler point target response (eq. 15) times delta_fn.  Stored delay fastest.
SMRT_DEV void sar_h14_doppler_row(const SarBatch& b, int n, int tid, int nt, unsigned char* lds) {
    const int ND = b.ND;
    double* phi = (double*)lds;
    double* F = phi + ND;
    double* g = F + ND;
    const double tau = sar_tau(b, n), h = b.lrm.altitude;
    const double rho2 = h * tau / b.alpha * kCSpeed;
    for (int c = tid; c < ND; c += nt) {
        const double fn = sar_doppler_frequency(b, c);
        const double yn = h * b.wavelength / (2.0 * b.velocity) * fn;
        const double xn = rho2 - yn * yn;
        phi[c] = xn > 0.0 ? atan(yn / sqrt(xn)) : NAN;
        g[c] = sar_sinc2(fn / (b.prf / b.ndoppler));
    }
    lrm_sync();
    const double pref = b.h14_pu / kPi * exp(-4.0 * kCSpeed * tau / (b.alpha * b.h14_gamma * h));
    for (int c = tid; c < ND; c += nt) {
        const double d = c < ND - 1 ? phi[c + 1] - phi[c] : phi[0] - phi[1];
        const double f = pref * d;
        F[c] = f != f ? 0.0 : f;
    }
    lrm_sync();
    const int s = (ND - 1) / 2;
    const double delta_fn = b.prf / ND;
    for (int c = tid; c < ND; c += nt) {
        const int lo = c + s - (ND - 1) > 0 ? c + s - (ND - 1) : 0, hi = c + s < ND - 1 ? c + s : ND - 1;
        double acc = 0.0;
        for (int k = lo; k <= hi; ++k) acc += F[k] * g[c + s - k];
        b.h14_doppler[(size_t)c * b.N_wide + n] = acc * delta_fn;
    }
}

// One workgroup per table: the time point target response (eq. 6) on the reference's 2 (N / 2) - 1 samples, convolved with the
// Gaussian height distribution (eq. 5) sampled on the same points when sigma_surface > 0 -- also where it is narrower than the
// sample spacing and the samples no longer sum to one --, left alone when it is 0.
SMRT_DEV void sar_h14_kernel_table(const SarBatch& b, int t, int tid, int nt, unsigned char* lds) {
    const int M = b.M, half = b.lrm.N / 2;
    double* p = (double*)lds;
    double* q = p + M;
    const double dtau = 1.0 / (b.lrm.os * b.lrm.bandwidth), ss = 2.0 * b.tab_sigma[t] / kCSpeed;
    const bool rough = b.tab_sigma[t] > 0.0;
    for (int j = tid; j < M; j += nt) {
        const double ct = (double)(j - half + 1) * dtau;
        p[j] = sar_sinc2(ct / (1.0 / b.lrm.bandwidth));
        q[j] = rough ? exp(-(ct * ct) / (2.0 * ss * ss)) / (sqrt(2.0 * kPi) * ss) : 0.0;
    }
    lrm_sync();
    for (int m = tid; m < M; m += nt) {
        double acc = p[m];
        if (rough) {
            const int c = m + half - 1;   // p[j] q[c - j]
            const int lo = c - (M - 1) > 0 ? c - (M - 1) : 0, hi = c < M - 1 ? c : M - 1;
            acc = 0.0;
            for (int j = lo; j <= hi; ++j) acc += p[j] * q[c - j];
            acc *= dtau;
        }
        b.h14_kernel[(size_t)t * M + m] = acc;
    }
}

// One workgroup per (table, Doppler column): the convolution along the delay (eq. 7) times dtau, times Nb / prf, and the delay
// compensation (eq. 19): the column moves floor(idelta_r1 (c - Nb / 2 + 0.5)^2) rows up, zeros come in below, and a column whose
// shift reaches N_wide is all zero.  Only the first N rows are kept.
SMRT_DEV void sar_h14_delay_column(const SarBatch& b, int t, int c, int tid, int nt, unsigned char* lds) {
    const int N = b.lrm.N, NW = b.N_wide, M = b.M, half = N / 2;
    double* a = (double*)lds;
    double* k = a + NW;
    for (int j = tid; j < NW; j += nt) a[j] = b.h14_doppler[(size_t)c * NW + j];
    for (int m = tid; m < M; m += nt) k[m] = b.h14_kernel[(size_t)t * M + m];
    lrm_sync();
    const double off = (double)(c - b.ND / 2) + 0.5;
    const double up = b.slant ? floor(b.idelta_r1 * (off * off)) : 0.0;
    const int shift = up < (double)NW ? (int)up : NW;
    const double scale = 1.0 / (b.lrm.os * b.lrm.bandwidth) * ((double)b.ND / b.prf);
    double* tab = b.tables + ((size_t)t * b.ND + c) * N;
    for (int n = tid; n < N; n += nt) {
        const int r = n + shift;
        double acc = 0.0;
        if (r < NW) {
            const int e = r + half - 1;   // a[j] k[e - j]
            const int lo = e - (M - 1) > 0 ? e - (M - 1) : 0, hi = e < NW - 1 ? e : NW - 1;
            for (int j = lo; j <= hi; ++j) acc += a[j] * k[e - j];
        }
        tab[n] = acc * scale;
    }
}

// ---- the map ----------------------------------------------------------------------------------------------------------------
// LDS of the kernel: v [N]; D, P1, V, W [osd][N] doubles (Halimi14: no P1)
inline size_t sar_combine_lds_bytes(int N, int osd) { return (size_t)N * (1 + 4 * (size_t)osd) * sizeof(double); }

// MODEL is where the fine columns of a pair come from and how a boundary weighs them: kSarDinardo18, D and P1 of D18 eq. 22 from
// the f0 / f1 tables, a boundary at its own nu; kSarHalimi14, the pair's table as it is, the same for every boundary.
template <int MODEL>
SMRT_DEV void sar_combine_model(const SarBatch& b, long long i, int bin, int tid, int nt, unsigned char* lds) {
    const LrmBatch& lb = b.lrm;
    const long long gp = lrm_global_pair(lb, i);
    const int s = (int)(gp % lb.fo.S);
    const int L = lb.fo.n_layers[s], Lmax = lb.fo.Lmax, N = lb.N, osd = b.osd, ND = b.ND, ost = lb.os;
    const bool oversampled = lb.oversampled != 0;
    double* v = (double*)lds;
    double* D = v + N;
    double* P1 = D + (size_t)osd * N;
    double* V = P1 + (MODEL == kSarDinardo18 ? (size_t)osd * N : 0);   // the convolution with the volume backscatter, made once for its row and for the total
    double* W = V + (size_t)osd * N;
    double* out = b.out + (size_t)i * b.out_rows * b.n_t * b.n_d;
    if (lb.status[i] != ST_OK) {
        const int cols = oversampled ? osd : 1;
        for (int k = tid; k < b.out_rows * b.n_t * cols; k += nt) {
            const int r = k / (b.n_t * cols), n = (k / cols) % b.n_t, c = k % cols;
            out[((size_t)r * b.n_t + n) * b.n_d + (size_t)bin * cols + c] = NAN;
        }
        return;
    }
    if constexpr (MODEL == kSarHalimi14) {
        const double* tab = b.tables + ((size_t)b.tab_index[s] * ND + (size_t)bin * osd) * N;   // the osd columns are contiguous
        for (int idx = tid; idx < osd * N; idx += nt) D[idx] = tab[idx];
    } else {
        const double ss = b.tab_sigma[b.tab_index[s]];
        const double* tab = b.tables + (size_t)b.tab_index[s] * 2 * N * ND;
        // (dinardo18.py computes the tanh term of D18 eq. 26 and discards it: a constant correction for roll > 0, none otherwise)
        const double tk0 = 1.0 - (b.roll > 0.0 ? b.roll * (2.0 * b.gamma_y * b.roll) : 0.0);
        for (int idx = tid; idx < osd * N; idx += nt) {
            const int cc = idx / N, n = idx % N, c = bin * osd + cc;
            const double look = sar_look_angle(b, c), sigma_c = sar_sigma_c(b, look, ss), f = sar_f(b, n);
            const double gl = 1.0 / lb.bandwidth / sigma_c, dp = look - b.pitch;
            const double gamma_kl = exp(-b.gamma_y * b.roll * b.roll - b.gamma_x * (dp * dp) - b.gamma_y * f) * cosh(2.0 * b.gamma_y * b.roll * sqrt(f));
            const double pref = b.pu * gamma_kl / sqrt(sigma_c);
            const double p1 = pref * (ss / b.l_gamma * gl * (ss / b.lz)) * tab[(size_t)N * ND + (size_t)n * ND + c];
            P1[idx] = p1;
            D[idx] = pref * tab[(size_t)n * ND + c] + tk0 * p1;
        }
    }
    for (int n = tid; n < N; n += nt) v[n] = lb.vsd[(size_t)i * N + n];
    lrm_sync();
    const int* map = b.row_map + (size_t)s * (2 * (Lmax + 1) + 2);
    const int total_row = map[2 * (Lmax + 1) + 1];
    for (int idx = tid; idx < osd * N; idx += nt) {
        const int cc = idx / N, n = idx % N;
        const double* d = D + (size_t)cc * N;
        double acc = 0.0;
        for (int k = 0; k <= n; ++k) acc += d[n - k] * v[k];
        V[idx] = acc;
    }
    const double* e = b.echo + i * (Lmax + 1) * SAR_ECHO;
    const double* bv = lb.itf + gp * (Lmax + 1) * SAR_BV;
    for (int r = 0; r < b.out_rows; ++r) {
        const bool total = r == total_row, volume = total || map[2 * (Lmax + 1)] == r;
        for (int idx = tid; idx < osd * N; idx += nt) {
            const int cc = idx / N, n = idx % N;
            const double* d = D + (size_t)cc * N;
            const double* p1 = P1 + (size_t)cc * N;
            double acc = volume ? V[idx] : 0.0;
            const double look = sar_look_angle(b, bin * osd + cc);
            for (int k = 0; k <= L; ++k)
                for (int coherent = 0; coherent < 2; ++coherent) {
                    if (!total && map[coherent * (Lmax + 1) + k] != r) continue;
                    const double echo = e[k * SAR_ECHO + (coherent ? SAR_ECHO_COHERENT : SAR_ECHO_INCOHERENT)];
                    const int m = n - (int)e[k * SAR_ECHO + SAR_ECHO_SHIFT];
                    if (!(echo > 0.0) || m < 0) continue;
                    if constexpr (MODEL == kSarHalimi14) {
                        acc += echo * d[m];
                    } else {
                        const double nu = coherent ? b.nu_coherent : bv[k * SAR_BV + SAR_BV_NU];
                        acc += echo * (exp(-nu * (look * look) - nu * sar_f(b, m)) * (d[m] + nu / b.gamma_y * p1[m]));
                    }
                }
            W[idx] = acc;
        }
        lrm_sync();
        double* row = out + (size_t)r * b.n_t * b.n_d;
        if (oversampled) {
            for (int idx = tid; idx < osd * N; idx += nt) row[(size_t)(idx % N) * b.n_d + (size_t)bin * osd + idx / N] = W[idx];
        } else {
            for (int g = tid; g < lb.ngate; g += nt) {
                double acc = 0.0;
                for (int k = 0; k < ost; ++k)
                    for (int cc = 0; cc < osd; ++cc) acc += W[(size_t)cc * N + g * ost + k];
                row[(size_t)g * b.n_d + bin] = acc / (ost * osd);
            }
        }
        lrm_sync();
    }
}

SMRT_DEV void sar_combine_item(const SarBatch& b, long long i, int bin, int tid, int nt, unsigned char* lds) {
    sar_combine_model<kSarDinardo18>(b, i, bin, tid, nt, lds);
}

}  // namespace smrt
