// The per-layer prep of the LDS-resident passive pipelines (N <= 64): what MODE 1 of dort_pair_passive does with one
// workgroup per pair and the LDS of the largest layer a batch may have, split into
//   - a pair setup kernel (one wavefront per pair): pair_setup -- layer scalars, process_coherent_layers, the most refringent
//     layer, stream counts -- and per kept layer of this round a RECORD in the staging area (DevStage::rec): streams, ke, ks,
//     pa, pb, pc, index in the input, stream cosines and weights; it also writes the row count to stg.n[item] and the
//     pair's status (a pair it rejects gets the rows and the code fail_pair gives it in the per-pair kernel);
//   - a layer kernel, one workgroup per (pair, layer) item and one launch per size class of rows (the eigensolver's:
//     (0, 32], (32, 48], (48, 64]; an item of another class leaves at once), with the LDS of one layer of the class
//     (make_plan slim = 4): assembly, renormalisation, X+-, the two Cholesky factorisations, B = L+^T L-, the staging
//     writes.  The arithmetic of a layer and the order of every sum are those of the per-pair kernel: the staging area is
//     bitwise the same.
// The layers of a pair do not depend on each other here; what does need them in order -- prune_mark_pair, the running
// optical depth from the top -- still runs after the diagonalisation of a round, as with the per-pair kernel.
// Part of the DORT device code (see dort_device.hpp for the overview and the reference map).
#pragma once
#include "dort_class_lists.hpp"
#include "dort_passive.hpp"

namespace smrt {

// cosine of stream j in a layer of relative index ri (streams.py:136-223), and the weight of stream j of n (streams.py:324-330):
// the expressions of dort_pair_passive, from the tables of pair_setup
SMRT_DEV double prep_stream_mu(const Lds& s, int l, int j) { const double rs = s.ri[l] * s.gsin[j]; return sqrt(1.0 - rs * rs); }
SMRT_DEV double prep_stream_weight(const Lds& s, int l, int j, int n) {
    double w;
    if (j == 0) w = 1.0 - 0.5 * (prep_stream_mu(s, l, 0) + prep_stream_mu(s, l, 1));
    else if (j == n - 1) w = fabs(0.5 * (prep_stream_mu(s, l, n - 2) + prep_stream_mu(s, l, n - 1)));
    else w = fabs(0.5 * (prep_stream_mu(s, l, j - 1) - prep_stream_mu(s, l, j + 1)));
    return w;
}

// ---- pair setup: one small workgroup per pair -------------------------------------------------------------------------
template <int NT>
SMRT_DEV void dort_prep_setup_pair(const DevBatch& b, long long p, double* lds_base, const DevStage& stg) {
    const int t = tid();
    const LdsPlan plan = make_plan(b.n_max_stream, 2, b.Lmax, b.n_theta, 9, 1, 0, 5);
    Lds s = carve(lds_base, lds_base, plan);
    const int nmax = b.n_max_stream;
    const long long gp = global_pair(b, p);
    const int fi = (int)(gp / b.S), si = (int)(gp % b.S);
    const double frequency = b.frequency[fi];
    int L = b.n_layers[si];
    if (t < 8) s.ints[t] = 0;
    block_sync();
    {
        const long long o = (long long)si * b.Lmax;
        const int st = pair_setup<NT>(b, s, frequency, L, b.thickness + o, b.frac_volume + o, b.temperature + o, b.p1 + o, b.p2 + o,
                                      b.layer_kind ? b.layer_kind + o : nullptr, gp);
        if (st != ST_OK) { fail_pair<NT>(b, p, st, 2 * b.n_theta); return; }
        L = s.ints[6];   // fewer than the snowpack's under process_coherent_layers
    }
    if (b.pair_done && b.pair_done[p]) return;   // the cut of this pair lies above this round's layers (uniform)
    for (int l = 0; l < L; ++l) {
        if (l < b.layer_lo || l >= b.layer_hi) continue;   // not in this round
        const long long item = p * (long long)b.Lmax + l;
        double* rec = stg.rec + item * stg.rec_stride;
        const int n = (int)s.nl[l];
        for (int j = t; j < n; j += NT) {
            rec[kPrepRecHead + j] = prep_stream_mu(s, l, j);
            rec[kPrepRecHead + nmax + j] = prep_stream_weight(s, l, j, n);
        }
        if (t == 0) {
            rec[kPrepRecN] = (double)n; rec[kPrepRecKe] = s.ks[l] + s.ka[l]; rec[kPrepRecKs] = s.ks[l];
            rec[kPrepRecPa] = s.pa[l]; rec[kPrepRecPb] = s.pb[l]; rec[kPrepRecPc] = s.pc[l]; rec[kPrepRecLo] = s.lo[l];
            stg.n[item] = setup_item_rows(s, l);   // 2 n, the layer kernel's size class (and what the class lists of the upload were built from); it replaces it by -status where the layer fails
        }
    }
    if (t == 0) b.status[p] = ST_OK;
}

// rows of a staging item for the class filter of the layer kernel (like eig_item_rows): 0 beyond the snowpack, for a pair
// the setup kernel rejected, and where nothing was staged in this round
SMRT_DEV int prep_item_rows(const DevBatch& b, const DevStage& stg, long long item) {
    const long long p = item / b.Lmax;
    const int l = (int)(item % b.Lmax);
    const int si = (int)(global_pair(b, p) % b.S);
    if (l >= b.n_layers[si] || b.status[p] != ST_OK) return 0;
    if (b.pair_done && b.pair_done[p]) return 0;
    const int n = stg.n[item];
    return (n > 0 && n <= stg.vec_stride) ? n : 0;
}

// ---- one (pair, layer) item of at most HI rows ------------------------------------------------------------------------
template <int NT, int HI>
SMRT_DEV void dort_prep_layer_item(const DevBatch& b, const DevStage& stg, long long item, double* lds_base) {
    const int t = tid();
    const int nphi = 9;  // m_max = 0 -> 16 azimuth samples (emmodel/common.py:401-414), 9 distinct by symmetry
    const LdsPlan plan = make_plan(HI / 2, 2, 0, 0, nphi, 1, 0, 4);
    Lds s = carve(lds_base, lds_base, plan);
    const int LD = plan.LD;                                        // of the packed triangles in LDS: the class's
    const int LDG = (int)(stg.mat_stride / stg.vec_stride);        // of the matrices in the staging area: the batch's
    const long long p = item / b.Lmax;
    const long long gp = global_pair(b, p);
    const int si = (int)(gp % b.S);
    const double* rec = stg.rec + item * stg.rec_stride;
    const int n = (int)rec[kPrepRecN], N = 2 * n;
    const double ke = rec[kPrepRecKe], ks = rec[kPrepRecKs], pa = rec[kPrepRecPa], pb = rec[kPrepRecPb], pc = rec[kPrepRecPc];
    const int lo = (int)rec[kPrepRecLo];   // the layer's index in the input arrays

    if (t < 8) s.ints[t] = 0;
    for (int k = t; k < nphi; k += NT) {  // azimuth table of the phase-matrix assembly
        const double ph = kPi * (double)k / (double)(nphi - 1);
        const double c = cos(ph), sn = sin(ph);
        s.cphi[k] = c; s.s2phi[k] = sn * sn;
        s.wphi[k] = ((k == 0 || k == nphi - 1) ? 1.0 : 2.0) / (double)(2 * (nphi - 1));
    }
    for (int j = t; j < n; j += NT) {   // per-row copies of the cosines and weights (the stream vectors stay in the record)
        const double m = rec[kPrepRecHead + j], w = rec[kPrepRecHead + b.n_max_stream + j];
        s.mrow[2 * j] = m; s.mrow[2 * j + 1] = m;
        s.wrow[2 * j] = w; s.wrow[2 * j + 1] = w;
    }
    block_sync();
    auto layer_failed = [&](int code) { if (t == 0) stg.n[item] = -code; };
    // (a layer the Rayleigh kernel will diagonalise in closed form needs neither matrix: see dort_pair_passive)
    const bool ray_direct = b.rayleigh_direct && stg.Linv && em_has_rayleigh_phase((int)pc & 15);   // (uniform)
    // -- phase matrix, azimuth mode 0.  The loop over the stream pairs is the per-pair kernel's: sharing its last partial
    //    round among the wavefronts would not shorten it (a wavefront with one active lane takes as long as a full one),
    //    and splitting the azimuth sum of an entry across lanes would change the order of that sum.
    if (!ray_direct) {
        const int T = n * (n + 1) / 2;
        const int em_l = (int)pc & 15, ms_l = (int)pc >> 4;   // this layer's emmodel and microstructure
        const long long o = (long long)si * b.Lmax + lo;
        const double fv = b.frac_volume[o], q1 = b.p1[o], q2 = b.p2[o];
        const double krho = __builtin_expect(ms_l >= MS_EXPC, 0) ? pc - (double)(int)pc : 0.0;   // Im / Re of k^2 (pair_setup)
        for (int idx = t; idx < T; idx += NT) {
            int i = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
            while ((i + 1) * (i + 2) / 2 <= idx) ++i;
            while (i * (i + 1) / 2 > idx) --i;
            const int j = idx - i * (i + 1) / 2;
            phase_mode0_block<true>(b, gp, lo, em_l, ms_l, pa, pb, fv, q1, q2, krho, s.cphi, s.s2phi, s.wphi, nphi, i, j,
                                    s.mrow[2 * i], s.mrow[2 * j], s.M0, s.M1, LD);
        }
    }
    block_sync();
    // -- energy-conserving renormalisation (dort.py:782-819): norm_r = ks / (c sum_c S+[r,c] w_c), c = 1/2
    for (int r = t; r < N; r += NT) {
        double rs = 0.0;
        if (ray_direct) {   // the two sums over the streams of dort_pair_passive
            double W0 = 0.0, W2 = 0.0;
            for (int j = 0; j < n; ++j) { const double wj = s.wrow[2 * j], mj = s.mrow[2 * j]; W0 += wj; W2 += wj * mj * mj; }
            const double a2 = s.mrow[r] * s.mrow[r];
            rs = pa * ((r & 1) ? (W2 + W0) : (a2 * W2 + 2.0 * (1.0 - a2) * (W0 - W2) + a2 * W0));
        } else {
            for (int c = 0; c <= r; ++c) rs += s.M0[sidx<true>(r, c, LD)] * s.wrow[c];
            for (int c = r + 1; c < N; ++c) rs += s.M0[sidx<true>(c, r, LD)] * s.wrow[c];
        }
        double nr = 1.0;
        if (b.normalization != 0 && ks != 0.0) {
            nr = ks / (0.5 * rs);
            if (b.normalization == 1 && !(fabs(nr - 1.0) <= 0.3)) lds_max(&s.ints[0], ST_NORM);
        }
        const double uu = sqrt(nr * s.wrow[r] / s.mrow[r]);
        s.u[r] = uu;
        s.d[r] = uu / s.wrow[r];
    }
    block_sync();
    if (s.ints[0] != ST_OK) { layer_failed(s.ints[0]); return; }
    if (ray_direct) {   // the scalars dort_rayleigh_kernel.hpp diagonalises the layer from (its header has the layout of the slot)
        double* gI = stg.Linv + item * stg.linv_stride;
        for (int r = t; r < N; r += NT) { gI[2 + n + r] = s.u[r]; stg.d[item * stg.vec_stride + r] = s.d[r]; }
        for (int j = t; j < n; j += NT) gI[2 + j] = s.mrow[2 * j];
        if (t == 0) { gI[0] = ke; gI[1] = pa; stg.n[item] = N + kStageDirect; }
        return;
    }
    // -- X+- = M^-1/2 T (ke I - c N S+- W) T^-1 M^-1/2, symmetric positive definite (lower triangles)
    for_2d<NT>(N, N, [&](int r, int c) {
        if (r >= c) {
            const double uu = 0.5 * s.u[r] * s.u[c];
            const double dg = (r == c) ? ke / s.mrow[r] : 0.0;
            s.M0[sidx<true>(r, c, LD)] = dg - uu * s.M0[sidx<true>(r, c, LD)];
            s.M1[sidx<true>(r, c, LD)] = dg - uu * s.M1[sidx<true>(r, c, LD)];
        }
    });
    block_sync();
    if (!chol2_mfma<NT, true>(s.M0, s.M1, s.gj, &s.ints[2], N, LD, stg.Linv ? stg.Linv + item * stg.linv_stride : nullptr)) {
        layer_failed(ST_ALBEDO);
        return;
    }
    // B = L+^T L- straight from the accumulators into the staging area
    lt_times_l_mfma<NT, true>(s.M0, s.M1, stg.B + item * stg.mat_stride, N, LD,
#ifdef SMRT_NO_COLUMN_REVERSAL
                              false,
#else
                              true,
#endif
                              LDG);
    // park L+ and d for the finish kernel
    double* gL = stg.L + item * stg.mat_stride;
    for_2d<NT>(N, N, [&](int r, int c) { gL[c * LDG + r] = (r < c) ? 0.0 : s.M0[sidx<true>(r, c, LD)]; });
    for (int r = t; r < N; r += NT) stg.d[item * stg.vec_stride + r] = s.d[r];
    if (t == 0) stg.n[item] = N;
}

}  // namespace smrt
