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
};

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

// ---- the map ----------------------------------------------------------------------------------------------------------------
// LDS of the kernel: v [N]; D, P1, V, W [osd][N] doubles
inline size_t sar_combine_lds_bytes(int N, int osd) { return (size_t)N * (1 + 4 * (size_t)osd) * sizeof(double); }

SMRT_DEV void sar_combine_item(const SarBatch& b, long long i, int bin, int tid, int nt, unsigned char* lds) {
    const LrmBatch& lb = b.lrm;
    const long long gp = lrm_global_pair(lb, i);
    const int s = (int)(gp % lb.fo.S);
    const int L = lb.fo.n_layers[s], Lmax = lb.fo.Lmax, N = lb.N, osd = b.osd, ND = b.ND, ost = lb.os;
    const bool oversampled = lb.oversampled != 0;
    double* v = (double*)lds;
    double* D = v + N;
    double* P1 = D + (size_t)osd * N;
    double* V = P1 + (size_t)osd * N;   // the convolution with the volume backscatter, made once for its row and for the total
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
                    const double nu = coherent ? b.nu_coherent : bv[k * SAR_BV + SAR_BV_NU];
                    acc += echo * (exp(-nu * (look * look) - nu * sar_f(b, m)) * (d[m] + nu / b.gamma_y * p1[m]));
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

}  // namespace smrt
