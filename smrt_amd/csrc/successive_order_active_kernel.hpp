// Successive-order-of-scattering solver, ACTIVE mode (backscatter order by order; the active branches of the reference's
// smrt/rtsolver/successive_order.py: successing_order, compute_next_order, prepare_layer_properties): the per-item
// arithmetic of its kernels.  Layer scalars and sublayer counts are so_layer_item's (successive_order_kernel.hpp).
//
//   soa_prep_item    one workgroup per (pair, layer, mode): the weighted phase matrix (1 / ke) c_m P_m w of mode m on the +-mu
//                    grid with THREE polarisations (ft_even_phase_mode), c_0 = 1/2, c_m = 1/4, stored TRANSPOSED and
//                    zero-padded to a multiple of 16 (D = 6 n directions, Dp = round16(6 n_max_stream)).  The mode-0 item
//                    also writes, per direction, e^(-dtau / mu) and the Fresnel power coefficients of the two interfaces of
//                    the layer with Re(r_V r_H*) for U (fresnel_RT3), and for layer 0 those of the air side of the surface.
//                    A Flat substrate reflects; nothing emits in active mode.
//   soa_sweep_pass   one workgroup of 256 threads per (pair, pass), all orders in one call.  Pass 0 is the coherent pass (no
//                    phase matrix, never stops), pass 1 + m is azimuth mode m.  The passes of a pair are independent: the
//                    stopping tolerance is relative_tolerance x the largest emerging radiance of MODE 0 at order 0, and at
//                    order 0 the profile is zero, so what emerges is exactly the specular reflection of the pass's own
//                    incident columns; those of a mode m >= 1 are twice mode 0's, a scaling that is exact in binary floating
//                    point.  Every pass therefore forms the tolerance from its own order 0 (halved for m >= 1), bit-equal to
//                    the reference's, and no value crosses workgroups.  Per order:
//                      (a) source product S[k][c][d] = sum_q W_m[d][q] mean[k][c][q] with v_mfma_f64_16x16x4_f64: the rows
//                          (sublayer k, column c) of a layer are FLATTENED into the M dimension, so a thin layer with C
//                          columns still fills the 16 rows of a tile; the means are staged in LDS (A operand), Wt is read
//                          from global memory with unit stride (B operand);
//                      (b) the reflections of the previous order at the interfaces, saved before the profile is overwritten;
//                      (c) the recurrences I <- I e + S (1 - e), one lane per (direction, column): threads 0..127 sweep down,
//                          threads 128..255 sweep up; order 0 injects the incident columns through the surface and adds
//                          their specular reflection to what emerges;
//                      (d) the largest emerging radiance (all air rows, all columns), the stopping rule, and the backscatter
//                          pick: for column (incident stream i, polarisation p) the three polarisations of outgoing stream i.
//   soa_combine_item one lane per output element: from every mode's orders (1 + [m > 0]) x the coherent pass's orders are
//                    subtracted -- for ALL orders, also after the mode stopped --, the modes are summed at the azimuth phi
//                    (add_intensity_mode), the total over the orders is appended, and the incident streams are interpolated
//                    linearly in the cosine to the incidence angles, with the reference's nadir node when one of them is
//                    steeper than the steepest stream.
//
// Direction index inside a layer of n streams: d < 3 n upward (stream d / 3, polarisation d % 3: V, H, U), 3 n <= d < 6 n
// downward.  Column c = (incident stream jj, incident polarisation p) = jj * npi + p; the incident streams are the one or two
// air streams that bracket each cos(theta_inc), as a sorted set.  Streams: 2 to 64 as in passive mode (LDS: 16 rows of
// Dp + 2 <= 386 doubles and a few vectors, under 56 KiB; the workspace is in global memory and chunked by the host).
// The same source is compiled by g++ (-DSMRT_HOST_EMU) for the CPU tests.
#pragma once
#include "dort_active.hpp"
#include "successive_order_kernel.hpp"

namespace smrt {

constexpr int kSoaThreads = 256;
// per (pair, layer) vectors of 3 n_max_stream doubles
enum { SOA_EXT = 0, SOA_RTOP, SOA_TTOP, SOA_RBOT, SOA_TBOT, SOA_VECS };

SMRT_HD int soa_dp(int n_max_stream) { return so_round16(6 * n_max_stream); }
SMRT_HD int soa_tile_ld(int n_max_stream) { return ((soa_dp(n_max_stream) + 31) & ~31) + 2; }   // so_tile_ld's rule: 2 mod 32
SMRT_HD int soa_lds_doubles(int n_max_stream) {   // tile, reduction, air cosines, incident powers, incident streams (ints), scalars
    return 16 * soa_tile_ld(n_max_stream) + kSoaThreads + 3 * n_max_stream + 8;
}
SMRT_HD int soa_max_columns(int npi, int n_theta, int n_max_stream) {
    return npi * (2 * n_theta < n_max_stream ? 2 * n_theta : n_max_stream);
}
// doubles of the workspace of ONE pass of a pair: profile [I][C][Dp], source [K][C][Dp], boundary [L][2][C][Dh], emerging [C][Dh]
SMRT_HD long long soa_pass_doubles(long long n_sub, long long n_lay, long long C, int n_max_stream) {
    return ((2 * n_sub + n_lay) * soa_dp(n_max_stream) + (2 * n_lay + 1) * 3 * n_max_stream) * C;
}

struct SoaBatch {
    SoBatch so;        // the layer kernel's batch.  so.theta: the incidence angles; so.vec [n_pairs][Lmax][SOA_VECS][3 nmax];
                       // so.wt [chunk_count][m_max + 1][Lmax][Dp][Dp]; so.ws / so.ws_off: (m_max + 2) passes per pair;
                       // so.out [n_pairs][3][3][n_theta][n_iter + 1]; so.maxrad [n_pairs][m_max + 2][n_iter] (NaN: not run);
                       // so.orders [n_pairs][m_max + 2]; so.srcterm unused
    int npi, m_max, Cmax, reserved;
    double phi;
    double* air;       // [n_pairs][2][3 nmax]: transmission into layer 0, reflection, of the air side of the surface
    double* back;      // [n_pairs][m_max + 2][n_iter][3][Cmax] backscatter picks of every pass
    int* inc;          // [n_pairs][1 + nmax]: number of incident streams, their indices
};

// The incident streams (prepare_incident_streams): outmu descending, i0 = number of streams steeper than the beam.
SMRT_HD int soa_incident_streams(const double* outmu, int n_air, const double* theta, int n_theta, int* list) {
    int n = 0;
    for (int i = 0; i < n_air; ++i) {
        int take = 0;
        for (int it = 0; it < n_theta && !take; ++it) {
            const double um = cos(theta[it]);
            int i0 = 0;
            while (i0 < n_air && outmu[i0] > um) ++i0;
            if (i0 == 0) take = i == 0;
            else if (i0 == n_air) take = i == n_air - 1;
            else take = i == i0 || i == i0 - 1;
        }
        if (take) list[n++] = i;
    }
    return n;
}

// ---- kernel (b): one workgroup per (pair, layer, mode) -------------------------------------------------------------------
template <int NT>
SMRT_DEV void soa_prep_item(const SoaBatch& a, long long i, int l, int m) {
    const SoBatch& b = a.so;
    const int t = tid();
    const long long gp = so_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const int L = b.n_layers[s];
    if (l >= L) return;
    for (int k = 0; k < L; ++k) if (so_stage(b, SO_KIND, k, i) < 0.0) return;   // the sweep kernel reports it
    const cplx estar = so_estar(b, i, L);
    const cplx el = cmk(so_stage(b, SO_EPS_RE, l, i), so_stage(b, SO_EPS_IM, l, i));
    const double ri = csqrt_(cdiv(estar, el)).re;
    const int ns = so_count_streams(b, ri);
    if (m == 0 && t == 0) {
        b.nstream[i * b.Lmax + l] = ns;
        b.layer_out[(i * b.Lmax + l) * 5 + 4] = (double)ns;
    }
    if (ns < 2) return;
    const long long at = (long long)s * b.Lmax + l;
    const double ks = so_stage(b, SO_KS, l, i), ka = so_stage(b, SO_KA, l, i), ke = ks + ka;
    const int Dh = 3 * b.nmax, Dp = soa_dp(b.nmax);
    const int n = 3 * ns;   // directions per hemisphere
    if (m == 0) {
        const int K = b.nsub[i * b.Lmax + l];
        double* vec = b.vec + (i * b.Lmax + l) * SOA_VECS * Dh;
        for (int j = t; j < ns; j += NT) {
            const double mu = so_mu(b, ri, j);
            const double e = exp(-(ke * b.thickness[at]) / (double)K / mu);
            const cplx eup = l > 0 ? cmk(so_stage(b, SO_EPS_RE, l - 1, i), so_stage(b, SO_EPS_IM, l - 1, i)) : cmk(1.0, 0.0);
            double R3[3], T3[3], Rb[3] = {0.0, 0.0, 0.0}, Tb[3] = {0.0, 0.0, 0.0};
            fresnel_RT3(el, eup, mu, R3, T3);
            if (l < L - 1) fresnel_RT3(el, cmk(so_stage(b, SO_EPS_RE, l + 1, i), so_stage(b, SO_EPS_IM, l + 1, i)), mu, Rb, Tb);
            else if (b.sub_kind == SUB_FLAT) {   // reflection only: what goes through is lost, nothing emits
                double lost[3];
                fresnel_RT3(el, cmk(b.sub_p1[gp], b.sub_p2[gp]), mu, Rb, lost);
            }
            for (int p = 0; p < 3; ++p) {
                vec[SOA_EXT * Dh + 3 * j + p] = e;
                vec[SOA_RTOP * Dh + 3 * j + p] = R3[p]; vec[SOA_TTOP * Dh + 3 * j + p] = T3[p];
                vec[SOA_RBOT * Dh + 3 * j + p] = Rb[p]; vec[SOA_TBOT * Dh + 3 * j + p] = Tb[p];
            }
        }
        if (l == 0) {   // the surface seen from the air, on the air streams
            const double ria = csqrt_(estar).re;
            const int n_air = so_count_streams(b, ria);
            double* air = a.air + i * 2 * Dh;
            for (int j = t; j < n_air; j += NT) {
                double R3[3], T3[3];
                fresnel_RT3(cmk(1.0, 0.0), el, so_mu(b, ria, j), R3, T3);
                for (int p = 0; p < 3; ++p) { air[3 * j + p] = T3[p]; air[Dh + 3 * j + p] = R3[p]; }
            }
        }
    }
    // the transposed weighted phase matrix of mode m: Wt[q][d] = (1 / ke) c_m P_m[d][q] w_q, zero outside the 6 ns directions
    double* wt = b.wt + (((i - b.chunk_begin) * (a.m_max + 1) + m) * b.Lmax + l) * (long long)Dp * Dp;
    const int n16 = so_round16(2 * n);
    for (int idx = t; idx < n16 * n16; idx += NT) wt[(long long)(idx / n16) * Dp + idx % n16] = 0.0;
    block_sync();
    const int kind = (int)so_stage(b, SO_KIND, l, i);
    const int em = kind & 15, ms = kind >> 4;
    if (em == EM_NONSCAT || ks == 0.0) return;
    const double pa = so_stage(b, SO_PA, l, i), pb = so_stage(b, SO_PB, l, i);
    const double fv = b.frac_volume[at], p1 = b.p1[at], p2 = b.p2 ? b.p2[at] : 0.0;
    const double invke = 1.0 / ke, coef = m == 0 ? 0.5 : 0.25;
    for (int idx = t; idx < 4 * ns * ns; idx += NT) {
        const int fs = idx / (2 * ns), fi = idx % (2 * ns);   // scattered / incident stream of the full (+mu, -mu) grid
        const int js = fs < ns ? fs : fs - ns, ji = fi < ns ? fi : fi - ns;
        const double mus = fs < ns ? so_mu(b, ri, js) : -so_mu(b, ri, js);
        const double mui = fi < ns ? so_mu(b, ri, ji) : -so_mu(b, ri, ji);
        double e[3][3];
        ft_even_phase_mode(em, ms, pa, pb, fv, p1, p2, mus, mui, m, 3, b.nsamp, e);
        const double w = so_weight(b, ri, ji, ns);
        const int d0 = (fs < ns ? 0 : n) + 3 * js, q0 = (fi < ns ? 0 : n) + 3 * ji;
        for (int x = 0; x < 3; ++x)
            for (int c = 0; c < 3; ++c)
                wt[(long long)(q0 + c) * Dp + d0 + x] = invke * (coef * e[x][c]) * w;
    }
}

// ---- kernel (c): one workgroup per (pair, pass) ----------------------------------------------------------------------------
template <int NT>
SMRT_DEV void soa_sweep_pass(const SoaBatch& a, long long i, int pass, double* lds) {
    static_assert(NT == 256, "threads 0..127 sweep down, 128..255 sweep up");
    const SoBatch& b = a.so;
    const int t = tid();
    const long long gp = so_global_pair(b, i);
    const int s = (int)(gp % b.S);
    const int L = b.n_layers[s];
    const int Dh = 3 * b.nmax, Dp = soa_dp(b.nmax), LDm = soa_tile_ld(b.nmax);
    const int NO = b.n_iter, NP = a.m_max + 2, npi = a.npi, Cmax = a.Cmax;
    double* tile = lds;                       // [16][LDm]
    double* red = tile + 16 * LDm;            // [NT]
    double* outmu = red + NT;                 // [nmax]
    double* power = outmu + b.nmax;           // [nmax] incident radiance per incident stream of this pass
    int* incl = (int*)(power + b.nmax);       // [nmax] incident streams
    double* maxrad = b.maxrad + (i * NP + pass) * NO;
    double* back = a.back + (i * NP + pass) * (long long)NO * 3 * Cmax;
    // ---- validity, air streams --------------------------------------------------------------------------------------
    int bad = 0;
    for (int l = 0; l < L; ++l) if (so_stage(b, SO_KIND, l, i) < 0.0) bad = 1;
    const cplx estar = bad ? cmk(1.0, 0.0) : so_estar(b, i, L);
    const double ria = csqrt_(estar).re;
    const int n_air = bad ? 0 : so_count_streams(b, ria);
    int nsmax = 0;
    if (!bad) {
        for (int l = 0; l < L; ++l) {
            const int ns = b.nstream[i * b.Lmax + l];
            if (ns < 2) bad = 1;
            nsmax = ns > nsmax ? ns : nsmax;
        }
        if (n_air < 2) bad = 1;   // (the weight of an air stream is a finite difference of two cosines)
    }
    for (int it = 0; it < b.n_theta; ++it) { const double um = cos(b.theta[it]); if (!(um > 0.0 && um <= 1.0)) bad = 1; }
    if (bad) {
        for (int k = t; k < NO; k += NT) maxrad[k] = NAN;
        for (int k = t; k < NO * 3 * Cmax; k += NT) back[k] = NAN;
        if (pass == 0) {
            for (int k = t; k <= b.nmax; k += NT) { b.streams[i * (1 + b.nmax) + k] = 0.0; a.inc[i * (1 + b.nmax) + k] = 0; }
        }
        if (t == 0) { b.orders[i * NP + pass] = 0; if (pass == 0) b.status[i] = ST_INPUT; }
        return;
    }
    for (int j = t; j < n_air; j += NT) outmu[j] = so_mu(b, ria, j);
    block_sync();
    if (t == 0) {
        const int n_inc = soa_incident_streams(outmu, n_air, b.theta, b.n_theta, incl);
        red[0] = (double)n_inc;
    }
    block_sync();
    const int n_inc = (int)red[0];
    const int C = npi * n_inc;
    for (int jj = t; jj < n_inc; jj += NT)
        power[jj] = (pass > 1 ? 2.0 : 1.0) * (1.0 / (2.0 * kPi * so_weight(b, ria, incl[jj], n_air)));
    if (pass == 0) {
        for (int k = t; k <= b.nmax; k += NT) {
            b.streams[i * (1 + b.nmax) + k] = k == 0 ? (double)n_air : (k <= n_air ? outmu[k - 1] : 0.0);
            a.inc[i * (1 + b.nmax) + k] = k == 0 ? n_inc : (k <= n_inc ? incl[k - 1] : 0);
        }
    }
    // ---- workspace ----------------------------------------------------------------------------------------------------
    long long n_sub = 0;
    for (int l = 0; l < L; ++l) n_sub += b.nsub[i * b.Lmax + l];
    double* prof = b.ws + b.ws_off[i] + pass * soa_pass_doubles(n_sub, L, Cmax, b.nmax);   // [n_sub + L][C][Dp]
    double* src = prof + (n_sub + L) * C * Dp;                                              // [n_sub][C][Dp]
    double* bnd = src + n_sub * C * Dp;                                                      // [L][2][C][Dh]
    double* emg = bnd + (long long)L * 2 * C * Dh;                                           // [C][Dh]
    const double* wt0 = b.wt + ((i - b.chunk_begin) * (a.m_max + 1) + (pass > 0 ? pass - 1 : 0)) * b.Lmax * (long long)Dp * Dp;
    const double* vec0 = b.vec + i * b.Lmax * (long long)SOA_VECS * Dh;
    const double* air = a.air + i * 2 * Dh;
    const int lane = t & 63, wave = t >> 6;
    const int nj = 3 * nsmax, items = nj * C;
    double tol = 0.0;
    int order = 0;
    block_sync();
    for (; order < NO; ++order) {
        if (order > 0) {
            long long itop = 0, isub = 0;
            for (int l = 0; l < L; ++l) {
                const int K = b.nsub[i * b.Lmax + l], n2 = 6 * b.nstream[i * b.Lmax + l], n16 = so_round16(n2);
                if (pass > 0) {
                    // (a) the source of this order from the profile of the previous one; rows r = k C + c of the layer
                    const double* wt = wt0 + l * (long long)Dp * Dp;
                    const double* top = prof + itop * C * Dp;
                    const long long R = (long long)K * C;
                    for (long long r0 = 0; r0 < R; r0 += 16) {
                        for (int idx = t; idx < 16 * n16; idx += NT) {
                            const int rr = idx / n16, c = idx % n16;
                            const long long r = r0 + rr;
                            double v = 0.0;
                            if (r < R && c < n2) v = (top[r * Dp + c] + top[(r + C) * Dp + c]) / 2.0;
                            tile[rr * LDm + c] = v;
                        }
                        block_sync();
                        for (int dt = wave; dt < n16 / 16; dt += NT / 64) {
                            tile4 acc = tile_zero();
                            for (int q0 = 0; q0 < n16; q0 += 4) {
                                const int q = q0 + (lane >> 4);
                                mfma_tile(tile[(lane & 15) * LDm + q], wt[(long long)q * Dp + dt * 16 + (lane & 15)], acc);
                            }
                            for (int reg = 0; reg < 4; ++reg) {
                                const long long r = r0 + (lane >> 4) + 4 * reg;
                                if (r < R) src[(isub * C + r) * Dp + dt * 16 + (lane & 15)] = acc[reg];
                            }
                        }
                        block_sync();
                    }
                }
                // (b) specular reflection of the previous order at the two interfaces of the layer
                const int n = n2 / 2;
                const double* vec = vec0 + l * (long long)SOA_VECS * Dh;
                for (int idx = t; idx < n * C; idx += NT) {
                    const int j = idx % n, c = idx / n;
                    bnd[((2 * l) * C + c) * (long long)Dh + j] = vec[SOA_RTOP * Dh + j] * prof[(itop * C + c) * Dp + j];
                    bnd[((2 * l + 1) * C + c) * (long long)Dh + j] = vec[SOA_RBOT * Dh + j] * prof[((itop + K) * C + c) * Dp + n + j];
                }
                itop += K + 1; isub += K;
            }
            block_sync();
        }
        // (c) the two sweeps, one lane per (direction, column)
        const bool scatter = order > 0 && pass > 0;
        for (int item = t & 127; item < items; item += 128) {
            const int j = item % nj, c = item / nj;
            // the incident radiance of column c on air direction j (order 0 only)
            const double beam = (order == 0 && j == 3 * incl[c / npi] + c % npi) ? power[c / npi] : 0.0;
            if (t < 128) {
                double carry = (order == 0 && j < 3 * n_air) ? air[j] * beam : 0.0;
                long long itop = 0, isub = 0;
                for (int l = 0; l < L; ++l) {
                    const int K = b.nsub[i * b.Lmax + l], n = 3 * b.nstream[i * b.Lmax + l];
                    if (j < n) {
                        const double* vec = vec0 + l * (long long)SOA_VECS * Dh;
                        const double e = vec[SOA_EXT * Dh + j], ome = 1.0 - e;
                        double I = (order > 0 ? bnd[((2 * l) * C + c) * (long long)Dh + j] : 0.0) + carry;
                        prof[(itop * C + c) * Dp + n + j] = I;
                        for (int k = 0; k < K; ++k) {
                            const double sk = scatter ? src[((isub + k) * C + c) * Dp + n + j] : 0.0;
                            I = I * e + sk * ome;
                            prof[((itop + k + 1) * C + c) * Dp + n + j] = I;
                        }
                        carry = vec[SOA_TBOT * Dh + j] * I;
                    } else carry = 0.0;
                    itop += K + 1; isub += K;
                }
            } else {
                double carry = 0.0;
                long long itop = n_sub + L, isub = n_sub;
                for (int l = L - 1; l >= 0; --l) {
                    const int K = b.nsub[i * b.Lmax + l], n = 3 * b.nstream[i * b.Lmax + l];
                    itop -= K + 1; isub -= K;
                    if (j < n) {
                        const double* vec = vec0 + l * (long long)SOA_VECS * Dh;
                        const double e = vec[SOA_EXT * Dh + j], ome = 1.0 - e;
                        double I = (order > 0 ? bnd[((2 * l + 1) * C + c) * (long long)Dh + j] : 0.0) + carry;
                        prof[((itop + K) * C + c) * Dp + j] = I;
                        for (int k = K - 1; k >= 0; --k) {
                            const double sk = scatter ? src[((isub + k) * C + c) * Dp + j] : 0.0;
                            I = I * e + sk * ome;
                            prof[((itop + k) * C + c) * Dp + j] = I;
                        }
                        carry = vec[SOA_TTOP * Dh + j] * I;
                    } else carry = 0.0;
                }
                // (the air has no more streams than the first layer)
                if (j < 3 * n_air) emg[c * Dh + j] = order == 0 ? carry + air[Dh + j] * beam : carry;
            }
        }
        block_sync();
        // (d) the largest emerging radiance, the backscatter pick, the stopping rule (workgroup-uniform)
        double mine = -INFINITY;
        for (int idx = t; idx < 3 * n_air * C; idx += NT) {
            const double v = emg[(idx / (3 * n_air)) * Dh + idx % (3 * n_air)];
            mine = v > mine ? v : mine;
        }
        red[t] = mine;
        block_sync();
        for (int h = NT / 2; h > 0; h >>= 1) {
            if (t < h) red[t] = red[t + h] > red[t] ? red[t + h] : red[t];
            block_sync();
        }
        const double mx = red[0];
        for (int idx = t; idx < 3 * C; idx += NT) {
            const int x = idx / C, c = idx % C;
            back[((long long)order * 3 + x) * Cmax + c] = emg[c * Dh + 3 * incl[c / npi] + x];
        }
        if (t == 0) maxrad[order] = mx;
        if (tol == 0.0) tol = b.rtol * (pass > 1 ? mx / 2.0 : mx);
        block_sync();   // (red and emg are rewritten by the next order)
        if (pass > 0 && mx < tol) { ++order; break; }
    }
    for (long long k = t + (long long)order * 3 * Cmax; k < (long long)NO * 3 * Cmax; k += NT) back[k] = 0.0;
    for (int k = t + order; k < NO; k += NT) maxrad[k] = NAN;
    if (t == 0) { b.orders[i * NP + pass] = order; if (pass == 0) b.status[i] = ST_OK; }
}

// ---- kernel (d): one lane per output element ---------------------------------------------------------------------------
// Incident stream jj, scattered / incident polarisation x / p, order k (k == n_iter: the total): the modes summed at phi.
SMRT_DEV double soa_mode_sum(const SoaBatch& a, long long i, int x, int p, int jj, int k) {
    const int NO = a.so.n_iter, NP = a.m_max + 2;
    if (p >= a.npi) return 0.0;
    const int c = jj * a.npi + p;
    const double* back = a.back + i * NP * (long long)NO * 3 * a.Cmax;
    double total = 0.0;
    for (int o = (k == NO ? 0 : k); o < (k == NO ? NO : k + 1); ++o) {
        const long long at = ((long long)o * 3 + x) * a.Cmax + c;
        const double coh = back[at];
        double v = 0.0;
        for (int m = 0; m <= a.m_max; ++m) {
            const double im = back[(1 + m) * (long long)NO * 3 * a.Cmax + at] - coh * (m > 0 ? 2.0 : 1.0);
            if (m == 0) { if (x < 2 && p < 2) v += im; }
            else v += im * (x < 2 ? cos((double)m * a.phi) : sin((double)m * a.phi));
        }
        total += v;
    }
    return total;
}
// ... of the virtual node list: node -1 is the nadir node (mean co- and cross-polarised values of the steepest stream)
SMRT_DEV double soa_node(const SoaBatch& a, long long i, int x, int p, int node, int k) {
    if (node >= 0) return soa_mode_sum(a, i, x, p, node, k);
    if (x < 2 && p < 2) {
        if (x == p) return (soa_mode_sum(a, i, 0, 0, 0, k) + soa_mode_sum(a, i, 1, 1, 0, k)) / 2.0;
        return (soa_mode_sum(a, i, 1, 0, 0, k) + soa_mode_sum(a, i, 0, 1, 0, k)) / 2.0;
    }
    return soa_mode_sum(a, i, x, p, 0, k);
}
SMRT_DEV void soa_combine_item(const SoaBatch& a, long long i, int e) {
    const SoBatch& b = a.so;
    const int NO = b.n_iter, nt = b.n_theta;
    const int k = e % (NO + 1), it = (e / (NO + 1)) % nt, p = (e / ((NO + 1) * nt)) % 3, x = e / ((NO + 1) * nt * 3);
    double* out = b.out + i * 9LL * nt * (NO + 1);
    if (b.status[i] != ST_OK) { out[e] = NAN; return; }
    const int* inc = a.inc + i * (1 + b.nmax);
    const double* outmu = b.streams + i * (1 + b.nmax) + 1;
    const int n_inc = inc[0];
    double steepest = 0.0;
    for (int q = 0; q < nt; ++q) { const double u = cos(b.theta[q]); steepest = u > steepest ? u : steepest; }
    const int first = steepest > outmu[inc[1]] ? -1 : 0;   // the nadir node stands in front of the incident streams
    const int N = n_inc - first;
    const double um = cos(b.theta[it]);
    if (N == 1) { out[e] = soa_node(a, i, x, p, 0, k); return; }
    int q = first;
    while (q < n_inc - 2 && um < outmu[inc[1 + q + 1]]) ++q;
    const double x0 = q < 0 ? 1.0 : outmu[inc[1 + q]], x1 = outmu[inc[1 + q + 1]];
    const double y0 = soa_node(a, i, x, p, q, k), y1 = soa_node(a, i, x, p, q + 1, k);
    out[e] = y0 + (y1 - y0) * ((um - x0) / (x1 - x0));
}

}  // namespace smrt
