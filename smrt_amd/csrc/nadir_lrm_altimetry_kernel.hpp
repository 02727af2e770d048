// Nadir LRM altimetry solver (the reference's smrt/rtsolver/nadir_lrm_altimetry.py and lrm_waveform_model.py: Brown 1977,
// Newkirk & Brown 1992 for the Earth curvature, Lacroix et al. 2008, Larue et al. 2021): the arithmetic of its three kernels.
//
//   lrm_layer_item     one (pair, layer): the layer electromagnetics of the first-order solver (first_order_layer_item: the
//                      same staging rows, the same kinds) and the nadir backward scattering phase(-1, 1, pi)[0, 0] / 4 pi / eps.
//   lrm_vertical_pair  one workgroup per pair: the vertical scattering distribution.  Layer boundaries and sub-gates are both
//                      sorted, so they are MERGED BY RANK -- a gate finds its boundary count by binary search, a boundary its
//                      gate count in closed form (checked against the gates' counts) -- and the two prefix sums on the merged
//                      grid, of the two-way optical depth and of the attenuated backscatter, are wavefront scans with a carry
//                      across the wavefronts.  At equal depth a boundary precedes a gate.  Only the first ngate x oversampling
//                      sub-gates are made: a later one never reaches an output sample.
//   lrm_waveform_item  one workgroup per (pair, output row): Brown's flat surface impulse response on the device, the direct
//                      convolution in LDS, the mean over the sub-gates.
//
// With -DSMRT_HOST_EMU (g++, the CPU tests) a "workgroup" is one thread and a scan is a running sum: the same arithmetic in
// another order of additions.
#pragma once
#include "first_order_kernel.hpp"

namespace smrt {

constexpr double kEarthRadius = 6371000.0;
constexpr int kLrmThreads = 256;
// doubles per (pair, boundary) of the optional host-evaluated interfaces: the one-way transmission at nadir (NaN: Flat, on the
// device; -1: Transparent, on the device), then the echo per incidence sample
// rows of the per-pair layer prefix arrays [n_pairs][3][Lmax + 1]
enum { LRM_TLAY = 0, LRM_ZLAY, LRM_CUMTRANS, LRM_PREFIX_ROWS };

struct LrmBatch {
    FoBatch fo;                     // what first_order_layer_item reads and writes (stage, layer_out); n_theta unused
    int ngate, os, n_mu, shift;     // shift: sub-gates of the nominal gate (fast path)
    int contributions, oversampled, skip_pfs, N;   // N = ngate * os
    int rows, out_rows, n_out, sar; // rows of the vertical distribution; rows and samples per row of the waveform; sar: the
                                    // variant of nadir_sar_altimetry_kernel.hpp (0 in this solver)
    double altitude, bandwidth, gain, gamma, off_nadir, nominal_gate, pulse_sigma;
    const double* t_inc;            // [n_mu]
    const double *sigma_surface, *surface_slope;   // [S] or null
    const double* itf;              // [F * S][Lmax + 1][1 + n_mu] or null
    double* bs;                     // [Lmax][n_pairs] backward scattering / eps
    double* prefix;                 // [n_pairs][3][Lmax + 1]
    double* vsd;                    // [n_pairs][rows][N]
    double* out;                    // [n_pairs][out_rows][n_out]
    double* z_gate;                 // [n_pairs][n_out]
    int* status;                    // [n_pairs]
};

struct LrmLane { int tid, nt; double* wsum; };   // wsum: one double per wavefront (LDS)

#if defined(SMRT_HOST_EMU)
SMRT_DEV void lrm_sync() {}
template <bool MUL> SMRT_DEV double lrm_block_scan(const LrmLane&, double v, double& carry) {
    carry = MUL ? carry * v : carry + v;
    return carry;
}
#else
SMRT_DEV void lrm_sync() { __threadfence_block(); __syncthreads(); }
// the lane CTRL shifts to this one, or the identity of the operation where there is none / the row is masked out
template <int CTRL, int ROWMASK, bool MUL> SMRT_DEV double lrm_dpp(double v) {
    union { double d; int i[2]; } a, o, r;
    a.d = v; o.d = MUL ? 1.0 : 0.0;
    r.i[0] = __builtin_amdgcn_update_dpp(o.i[0], a.i[0], CTRL, ROWMASK, 0xF, false);
    r.i[1] = __builtin_amdgcn_update_dpp(o.i[1], a.i[1], CTRL, ROWMASK, 0xF, false);
    return r.d;
}
#define LRM_OP(a, b) (MUL ? (a) * (b) : (a) + (b))
template <bool MUL> SMRT_DEV double lrm_wave_scan(double v) {   // inclusive, 64 lanes
    v = LRM_OP(v, (lrm_dpp<0x111, 0xF, MUL>(v)));   // row_shr:1
    v = LRM_OP(v, (lrm_dpp<0x112, 0xF, MUL>(v)));   // row_shr:2
    v = LRM_OP(v, (lrm_dpp<0x114, 0xF, MUL>(v)));   // row_shr:4
    v = LRM_OP(v, (lrm_dpp<0x118, 0xF, MUL>(v)));   // row_shr:8
    v = LRM_OP(v, (lrm_dpp<0x142, 0xA, MUL>(v)));   // row_bcast:15 into rows 1 and 3
    v = LRM_OP(v, (lrm_dpp<0x143, 0xC, MUL>(v)));   // row_bcast:31 into rows 2 and 3
    return v;
}
// inclusive scan over the workgroup, continued from `carry` (which becomes the total); every thread calls it
template <bool MUL> SMRT_DEV double lrm_block_scan(const LrmLane& ln, double v, double& carry) {
    const double w = lrm_wave_scan<MUL>(v);
    const int wave = ln.tid >> 6, waves = ln.nt >> 6;
    if ((ln.tid & 63) == 63) ln.wsum[wave] = w;
    __syncthreads();
    double before = carry, total = carry;
    for (int k = 0; k < waves; ++k) {
        const double s = ln.wsum[k];
        if (k < wave) before = LRM_OP(before, s);
        total = LRM_OP(total, s);
    }
    __syncthreads();
    carry = total;
    return LRM_OP(before, w);
}
#undef LRM_OP
#endif

SMRT_DEV long long lrm_global_pair(const LrmBatch& b, long long i) { return b.fo.pair_map ? b.fo.pair_map[i] : i; }

// ---- kernel 1: one (pair, layer) -------------------------------------------------------------------------------------------
SMRT_DEV void lrm_layer_item(const LrmBatch& b, long long i, int l) {
    first_order_layer_item(b.fo, i, l);
    const double kindv = fo_stage(b.fo, FO_KIND, l, i);
    double bs = 0.0;
    if (kindv >= 0.0) {
        const int kind = (int)kindv;
        FoLayerPhase q;
        q.phase = kind & 15; q.ms = kind >> 4;
        q.pa = fo_stage(b.fo, FO_PA, l, i); q.pb = fo_stage(b.fo, FO_PB, l, i);
        q.fv = fo_stage(b.fo, FO_FV, l, i); q.p1 = fo_stage(b.fo, FO_P1, l, i); q.p2 = fo_stage(b.fo, FO_P2, l, i);
        const double ks = fo_stage(b.fo, FO_KS, l, i);
        if (q.phase == EM_HOST && ks != 0.0) fo_stage(b.fo, FO_KIND, l, i) = -2.0;   // no phase function to take the sample of
        else if (q.phase != EM_NONSCAT && q.phase != EM_HOST && ks != 0.0) bs = fo_phase(q, -1.0, 1.0).vv / fo_stage(b.fo, FO_EPS_RE, l, i);
        b.fo.layer_out[(i * b.fo.Lmax + l) * 5 + 4] = bs;
    }
    b.bs[(long long)l * b.fo.n_pairs + i] = bs;
}

// ---- kernel 2: the vertical scattering distribution of one pair ----------------------------------------------------------
// LDS of the kernel: zs, tauv [M] doubles; cumg [G] doubles; cnt, gidx [M] ints; nbg [G] ints, with M <= N + Lmax + 1, G <= N
inline size_t lrm_vertical_lds_bytes(int N, int Lmax) {
    const size_t M = (size_t)N + Lmax + 2;
    return (2 * M + N) * sizeof(double) + (2 * M + N) * sizeof(int) + 16 * sizeof(double);
}

struct LrmPrefix { const double *t, *z, *ct; };

// depth of the sub-gate at time tg (numpy.interp over the boundaries; at and after the last boundary: its depth); *j: the layer
SMRT_DEV double lrm_gate_depth(const LrmPrefix& p, int L, double tg, int* j) {
    if (tg >= p.t[L]) { *j = L; return p.z[L]; }
    int lo = 0, hi = L;                       // t[lo] <= tg < t[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.t[mid] <= tg) lo = mid; else hi = mid; }
    *j = lo;
    const double slope = (p.z[lo + 1] - p.z[lo]) / (p.t[lo + 1] - p.t[lo]);
    return slope * (tg - p.t[lo]) + p.z[lo];
}

SMRT_DEV void lrm_vertical_pair(const LrmBatch& b, long long i, const LrmLane& ln, unsigned char* lds) {
    const long long gp = lrm_global_pair(b, i);
    const int s = (int)(gp % b.fo.S);
    const int L = b.fo.n_layers[s], Lmax = b.fo.Lmax, N = b.N, tid = ln.tid, nt = ln.nt;
    const long long np = b.fo.n_pairs;
    const size_t Mcap = (size_t)N + Lmax + 2;
    double* zs = (double*)lds;
    double* tauv = zs + Mcap;
    double* cumg = tauv + Mcap;
    int* cnt = (int*)(cumg + N);
    int* gidx = cnt + Mcap;
    int* nbg = gidx + Mcap;
    double* pre = b.prefix + i * LRM_PREFIX_ROWS * (Lmax + 1);
    double* vsd = b.vsd + i * b.rows * N;
    double* zg = b.z_gate + i * b.n_out;
    // (the SAR variant: four doubles per boundary of which only the transmission is read here, no echo in the rows, the speed
    // of a layer from its complex permittivity, the first gate at 1e-25 m)
    const int itf_stride = b.sar ? 4 : 1 + b.n_mu;
    const double* itf = b.itf ? b.itf + gp * (Lmax + 1) * itf_stride : nullptr;
    const double step = b.bandwidth * b.os;     // sub-gates per second

    int bad = 0;
    for (int l = 0; l < L; ++l) if (fo_stage(b.fo, FO_KIND, l, i) < 0.0) bad = 1;
    if (bad) {
        for (int k = tid; k < b.rows * N; k += nt) vsd[k] = NAN;
        for (int k = tid; k < b.n_out; k += nt) zg[k] = NAN;
        if (tid == 0) b.status[i] = ST_INPUT;
        return;
    }
    // (every slot of the merged grid is filled below when the ranks are a permutation; a slot a rounding accident left out is a
    // gate-less, boundary-less point of layer 0 rather than an index read from uninitialised LDS)
    for (size_t k = tid; k < Mcap; k += nt) { zs[k] = 0.0; cnt[k] = 1; gidx[k] = -(1 << 30); }
    // A. the boundaries: two-way travel time, depth and cumulative two-way transmission, three scans over the layers
    {
        double ct = 0.0, cz = 0.0, cc = 1.0;
        for (int base = 0; base <= L; base += nt) {
            const int k = base + tid;
            double dt = 0.0, dz = 0.0, tt = 1.0;
            if (k >= 1 && k <= L) {
                const double e2 = fo_stage(b.fo, FO_EPS_RE, k - 1, i), e1 = k >= 2 ? fo_stage(b.fo, FO_EPS_RE, k - 2, i) : 1.0;
                dz = fo_stage(b.fo, FO_THICK, k - 1, i);
                dt = dz / (kCSpeed / (b.sar ? csqrt_(cmk(e2, fo_stage(b.fo, FO_EPS_IM, k - 1, i))).re : sqrt(e2)));
                double t1 = itf ? itf[(k - 1) * itf_stride] : NAN;
                if (t1 == -1.0) t1 = 1.0;
                else if (!(t1 == t1)) { double rv, rh; fresnel_RvRh(cmk(e1, 0.0), cmk(e2, 0.0), 1.0, &rv, &rh); t1 = 1.0 - rv; }
                tt = t1 * t1;
            }
            const double st = lrm_block_scan<false>(ln, dt, ct), sz = lrm_block_scan<false>(ln, dz, cz);
            const double sc = lrm_block_scan<true>(ln, tt, cc);
            if (k <= L) { pre[LRM_TLAY * (Lmax + 1) + k] = 2.0 * st; pre[LRM_ZLAY * (Lmax + 1) + k] = sz; pre[LRM_CUMTRANS * (Lmax + 1) + k] = sc; }
        }
    }
    lrm_sync();
    LrmPrefix p;
    p.t = pre + LRM_TLAY * (Lmax + 1); p.z = pre + LRM_ZLAY * (Lmax + 1); p.ct = pre + LRM_CUMTRANS * (Lmax + 1);
    // B. the gates: ng = max(ceil(t_L x step), 1) of them cover the snowpack; the first G <= N are made
    double ngd = ceil(p.t[L] * step);
    if (!(ngd >= 1.0)) ngd = 1.0;
    const int G = ngd + 1.0 < (double)N ? (int)ngd + 1 : N;
    const bool has_last = ngd + 1.0 <= (double)N;           // the pushed last gate is among them: index G - 1
    for (int g = tid; g < N; g += nt) {
        double z = NAN;
        if (g < G) {
            int j;
            z = lrm_gate_depth(p, L, (double)g / step, &j);
            if (b.sar && g == 0) z = 1e-25;
            if (has_last && g == G - 1) { int jj; z += 0.01 * (z - (b.sar && g == 1 ? 1e-25 : lrm_gate_depth(p, L, (double)(g - 1) / step, &jj))); }
            int nb = j + 1 > L + 1 ? L + 1 : j + 1;      // boundaries at or above the gate: a boundary precedes a gate at equal depth
            while (nb <= L && p.z[nb] <= z) ++nb;
            while (nb > 0 && p.z[nb - 1] > z) --nb;
            nbg[g] = nb;
            zs[g + nb] = z; cnt[g + nb] = nb; gidx[g + nb] = g;
        }
        if (b.oversampled) zg[g] = z;
        else if (g % b.os == 0) zg[g / b.os] = z;
    }
    lrm_sync();
    for (int k = tid; k <= L; k += nt) {
        double guess = ceil(p.t[k] * step);               // gates strictly above the boundary, in closed form ...
        int g = guess < 0.0 ? 0 : guess > (double)G ? G : (int)guess;
        while (g > 0 && nbg[g - 1] > k) --g;              // ... held to the gates' own counts
        while (g < G && nbg[g] <= k) ++g;
        if (g < G) { zs[k + g] = p.z[k]; cnt[k + g] = k + 1; gidx[k + g] = -1 - k; }
    }
    lrm_sync();
    const int M = G + nbg[G - 1];
    // C. two-way optical depth at every point of the merged grid
    {
        double carry = 0.0;
        if (tid == 0) tauv[0] = 0.0;
        for (int base = 0; base < M - 1; base += nt) {
            const int k = base + tid;
            double dtau = 0.0;
            if (k < M - 1) {
                const int lay = (cnt[k] < L ? cnt[k] : L) - 1;
                const double ke = fo_stage(b.fo, FO_KS, lay, i) + fo_stage(b.fo, FO_KA, lay, i);
                dtau = 2.0 * ke * (zs[k + 1] - zs[k]);
            }
            const double incl = lrm_block_scan<false>(ln, dtau, carry);
            if (k < M - 1) tauv[k + 1] = incl;
        }
    }
    lrm_sync();
    // D. the attenuated backscatter at every point, its prefix sum, the differences between the gates
    const bool split = b.rows > 1;
    const int n_scan = split ? b.n_mu + 1 : 1;          // interface rows, then the volume row; or the one row of everything
    for (int r = 0; r < n_scan; ++r) {
        const bool want_vol = !split || r == b.n_mu, want_itf = !split || r < b.n_mu;
        const int m = split ? (r < b.n_mu ? r : 0) : 0;
        double carry = 0.0;
        for (int base = 0; base < M; base += nt) {
            const int k = base + tid;
            double v = 0.0;
            if (k < M) {
                if (want_vol && k > 0) {
                    const int q = k - 1, c = cnt[q] < L ? cnt[q] : L, lay = c - 1;
                    const double ke = fo_stage(b.fo, FO_KS, lay, i) + fo_stage(b.fo, FO_KA, lay, i);
                    const double dtau = 2.0 * ke * (zs[k] - zs[q]);
                    v = (1.0 - exp(-dtau)) / (2.0 * ke) * b.bs[(long long)lay * np + i] * (exp(-tauv[q]) * p.ct[c]);
                }
                if (want_itf && !b.sar && gidx[k] < 0 && itf && !(split && k == 0)) {
                    const int bd = -1 - gidx[k];
                    const double e = bd <= L ? itf[bd * (1 + b.n_mu) + 1 + m] : 0.0;
                    if (e != 0.0) v += e * exp(-tauv[k]) * (k == 0 ? 1.0 : p.ct[cnt[k - 1] < L ? cnt[k - 1] : L]);
                }
            }
            const double incl = lrm_block_scan<false>(ln, v, carry);
            if (k < M && gidx[k] >= 0) cumg[gidx[k]] = incl;
        }
        lrm_sync();
        double* row = vsd + (split ? (r < b.n_mu ? b.n_mu + r : 2 * b.n_mu) : 0) * N;
        for (int g = tid; g < N; g += nt) row[g] = g < G ? cumg[g] - (g ? cumg[g - 1] : 0.0) : 0.0;
        lrm_sync();
    }
    if (split)   // the surface: the echo of boundary 0 in gate 0, one row per incidence sample
        for (int k = tid; k < b.n_mu * N; k += nt) vsd[k] = (k % N == 0 && itf) ? itf[1 + k / N] : 0.0;
    if (tid == 0) b.status[i] = ST_OK;
}

// ---- kernel 3: the waveform -------------------------------------------------------------------------------------------------
// modified Bessel function I0: the power series (all terms positive) up to 20, the asymptotic series beyond
SMRT_DEV double lrm_i0(double x) {
    x = fabs(x);
    if (x <= 20.0) {
        const double q = 0.25 * x * x;
        double term = 1.0, sum = 1.0;
        for (int k = 1; k < 500; ++k) {
            term *= q / ((double)k * (double)k);
            sum += term;
            if (term < 1e-17 * sum) break;
        }
        return sum;
    }
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 60; ++k) {
        const double odd = 2.0 * k - 1.0;
        term *= odd * odd / (8.0 * x * k);
        if (term < 1e-17) break;
        sum += term;
    }
    return exp(x) / sqrt(2.0 * kPi * x) * sum;
}

// Brown's flat surface impulse response with the Earth curvature, at the time otau after the surface (lrm_waveform_model.py: PFS)
SMRT_DEV double lrm_pfs(const LrmBatch& b, double wavelength, double otau, double slope) {
    const double e = kCSpeed / (b.altitude * (1.0 + b.altitude / kEarthRadius)) * otau;
    const double coef = b.gain * b.gain * (wavelength * wavelength) * kCSpeed / (4.0 * ((4.0 * kPi) * (4.0 * kPi)) * (b.altitude * b.altitude * b.altitude));
    const double theta = b.off_nadir + slope;
    if (theta == 0.0) {
        const double x = -4.0 / b.gamma * e;
        return coef * (x <= 0.0 ? exp(x) : 0.0);
    }
    const double st = sin(theta), x = -4.0 / b.gamma * (st * st + e * cos(2.0 * theta));
    const double bessel = lrm_i0(4.0 / b.gamma * sqrt(e > 0.0 ? e : 0.0) * sin(2.0 * theta));
    return coef * (x <= 0.0 ? exp(x) : 0.0) * bessel * (e >= 0.0 ? 1.0 : 0.0);
}

// LDS of the kernel: h, x, w [N] doubles; on the slow path dxs, xi [N] doubles and seg [N] ints
inline size_t lrm_waveform_lds_bytes(int N, int n_mu) {
    return (size_t)N * (3 * sizeof(double) + (n_mu > 1 ? 2 * sizeof(double) + sizeof(int) : 0));
}

// numpy.interp of the n_mu samples f (stride fs) at the precomputed segment: seg < 0: left of the samples (0), seg == n_mu - 1: at
// or right of the last one
SMRT_DEV double lrm_interp(const LrmBatch& b, const double* f, int fs, int seg, double dx) {
    if (seg < 0) return 0.0;
    if (seg >= b.n_mu - 1) return f[(b.n_mu - 1) * fs];
    const double slope = (f[(seg + 1) * fs] - f[seg * fs]) / (b.t_inc[seg + 1] - b.t_inc[seg]);
    return slope * dx + f[seg * fs];
}

SMRT_DEV void lrm_waveform_item(const LrmBatch& b, long long i, int row, const LrmLane& ln, unsigned char* lds) {
    const long long gp = lrm_global_pair(b, i);
    const int s = (int)(gp % b.fo.S);
    const int N = b.N, tid = ln.tid, nt = ln.nt;
    double* h = (double*)lds;
    double* x = h + N;
    double* w = x + N;
    double* dxs = w + N;
    double* xi = dxs + N;                     // slow path: the interface row of the first incidence sample
    int* seg = (int*)(xi + N);
    const double* vsd = b.vsd + i * b.rows * N;
    double* out = b.out + (i * b.out_rows + row) * b.n_out;
    if (b.status[i] != ST_OK) {
        for (int k = tid; k < b.n_out; k += nt) out[k] = NAN;
        return;
    }
    const double wavelength = kCSpeed / b.fo.frequency[gp / b.fo.S];
    const double slope = b.surface_slope ? b.surface_slope[s] : 0.0;
    const double step = b.bandwidth * b.os, t_nominal = b.nominal_gate / b.bandwidth;
    if (b.skip_pfs) {
        for (int n = tid; n < N; n += nt) w[n] = vsd[row * N + n];
    } else if (b.n_mu == 1) {
        // fast path: the impulse response convolved with the pulse and the surface height distribution in closed form, shifted by
        // the nominal gate, then ONE direct convolution with the row
        const double sigma_surface = b.sigma_surface ? b.sigma_surface[s] : 0.0;
        const double two_s = 2.0 * sigma_surface / kCSpeed, sigma_c = sqrt(b.pulse_sigma * b.pulse_sigma + two_s * two_s);
        for (int n = tid; n < N; n += nt) {
            const int src = n >= b.shift ? n - b.shift : 0;
            const double otau = (double)n / step - t_nominal;
            h[n] = lrm_pfs(b, wavelength, (double)src / step, slope) * (1.0 + erf(otau / (1.4142135623731 * sigma_c))) / 2.0 / b.bandwidth;
            x[n] = vsd[row * N + n];
        }
        lrm_sync();
        for (int n = tid; n < N; n += nt) {
            double acc = 0.0;
            for (int k = 0; k <= n; ++k) acc += h[n - k] * x[k];
            w[n] = acc;
        }
    } else {
        // slow path: the echo of the surface and of the interfaces follows the incidence angle across the waveform
        const int nm = b.n_mu;
        for (int n = tid; n < N; n += nt) {
            const double t = (double)n / step;
            h[n] = lrm_pfs(b, wavelength, t - t_nominal, slope);
            x[n] = vsd[2 * nm * N + n];
            xi[n] = vsd[nm * N + n];
            const double tq = t - t_nominal;
            int sg = -1;
            if (tq >= b.t_inc[nm - 1]) sg = nm - 1;
            else if (tq >= b.t_inc[0]) { sg = 0; while (sg < nm - 2 && b.t_inc[sg + 1] <= tq) ++sg; }
            seg[n] = sg;
            dxs[n] = sg >= 0 && sg < nm - 1 ? tq - b.t_inc[sg] : 0.0;
        }
        lrm_sync();
        const bool all = b.out_rows == 1;
        const double ptr = 1.0 / b.bandwidth;
        for (int n = tid; n < N; n += nt) {
            double ws = 0.0, wi = 0.0, wv = 0.0;
            if (all || row == 0) ws = lrm_interp(b, vsd + 0, N, seg[n], dxs[n]) * h[n];
            if (all || row == 2) { for (int k = 0; k <= n; ++k) wv += h[n - k] * x[k]; }
            if (all || row == 1)
                for (int k = 0; k <= n; ++k)
                    if (xi[k] > 0.0) wi += lrm_interp(b, vsd + nm * N + k, N, seg[n - k], dxs[n - k]) * h[n - k];
            w[n] = all ? ws * ptr + wi * ptr + wv * ptr : (row == 0 ? ws : row == 1 ? wi : wv) * ptr;
        }
    }
    lrm_sync();
    if (b.oversampled) { for (int n = tid; n < N; n += nt) out[n] = w[n]; return; }
    for (int g = tid; g < b.ngate; g += nt) {
        double acc = 0.0;
        for (int k = 0; k < b.os; ++k) acc += w[g * b.os + k];
        out[g] = acc / b.os;
    }
}

}  // namespace smrt
