// What the device batch of each solver beside DORT looks like, said once for the GPU entry points (the seven .hip units) and
// for the CPU builds of the same kernels (tests/hostemu/*_host.cpp): a describe function that fills every non-pointer field of
// the batch struct the kernels take by value from the C ABI inputs, and an extents function that gives, from a described
// batch, the element count of every buffer the kernels read or write and the LDS bytes their launches pass.  Plain C++: no
// HIP runtime call.  Pointers, the per-chunk fields (chunk_begin, chunk_count, wt, ws), grids, kernel order and chunk plans are
// NOT here: each .hip launches, and each driver loops, in its own words.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/smrt_dort.h"
#include "dort_host_common.hpp"
#include "first_order_kernel.hpp"
#include "multifresnel_kernel.hpp"
#include "nadir_lrm_altimetry_kernel.hpp"
#include "nadir_sar_altimetry_kernel.hpp"
#include "second_order_kernel.hpp"
#include "successive_order_active_kernel.hpp"
#include "successive_order_kernel.hpp"

namespace solver_describe {

// ---- what the batch structs name alike ---------------------------------------------------------------------------------------
template <class Batch>
void shape(Batch& d, const smrt_batch* b, int n_frequencies, int n_theta, int sub_kind, long long n_pairs) {
    d.S = b->n_snowpacks; d.Lmax = b->n_layers_max; d.F = n_frequencies; d.n_theta = n_theta;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.sub_kind = sub_kind;
    d.n_pairs = n_pairs;
}

// The smrt_batch arrays solver_host::upload_batch sends and tests/hostemu/host_batch.hpp binds, in elements: n_layers [S],
// the layer arrays [S][Lmax], frequency [F], each substrate array (0 without a substrate; the rough soils keep their [S][2]
// parameters behind the [F][S] permittivities, smrt_dort.h), the pair map (0 without one).
struct InputExtents { size_t snowpacks, layers, frequencies, substrate, pair_map; };
template <class Batch>
InputExtents inputs(const Batch& d, bool mapped) {
    const size_t S = d.S, F = d.F;
    return {S, S * d.Lmax, F, d.sub_kind == SMRT_SUBSTRATE_NONE ? 0 : F * S + (smrt_host::is_soil_substrate(d.sub_kind) ? 2 * S : 0),
            mapped ? (size_t)d.n_pairs : 0};
}
// ... and their bytes on the device (the optional arrays only where the batch has them)
inline size_t input_bytes(const smrt_batch* b, const InputExtents& in) {
    return in.snowpacks * sizeof(int32_t) + (5 + (b->liquid_water ? 1 : 0)) * in.layers * sizeof(double) +
           (b->layer_kind ? in.layers * sizeof(int32_t) : 0) + in.frequencies * sizeof(double) + 2 * in.substrate * sizeof(double) +
           in.pair_map * sizeof(int64_t);
}

// ---- first order -------------------------------------------------------------------------------------------------------------
inline smrt::FoBatch first_order(const smrt_batch* b, const smrt_first_order_extras* x, long long n_pairs) {
    smrt::FoBatch d{};
    shape(d, b, b->n_frequencies, b->n_theta, b->substrate_kind, n_pairs);
    if (x && x->host_interface_slot) d.n_slots = x->n_interface_slots;
    return d;
}
struct FoExtents {
    size_t theta, host_layer, host_coeff, itf_slot, itf_values, host_phase;            // inputs beside the smrt_batch arrays
    size_t stage, out, status, layer_out, layer_backscatter, diag, carry;
};
inline FoExtents extents(const smrt::FoBatch& d) {
    const size_t N = (size_t)d.n_pairs, L = d.Lmax, T = d.n_theta, FS = (size_t)d.F * d.S;
    return {T, FS * L * 4, FS * L, FS * (L + 1), FS * d.n_slots * T * smrt::kFoInterfaceDoubles, FS * L * T * 16,
            (size_t)smrt::FO_ROWS * L * N, N * 16 * T, N, N * L * 5, N * (L + 1) * T * 4, N * 2, N * L * T * smrt::kFoCarryDoubles};
}

// ---- second order: on top of first order, as its kernels are -----------------------------------------------------------------
inline smrt::So2Batch second_order(const smrt_batch* b, const smrt_second_order_extras* x, long long n_pairs) {
    smrt::So2Batch d{};
    d.fo = first_order(b, x ? x->first_order : nullptr, n_pairs);
    d.nmax = b->n_max_stream; d.m_max = b->m_max; d.nsamp = smrt::azimuth_samples(b->m_max);
    d.interlayer = (x && x->compute_scattering_interlayer) ? 1 : 0;
    return d;
}
struct So2Extents {
    size_t gl_mu, sub_modes, out, layer_backscatter;
    size_t nstream, streams, integ;   // the chunk buffers, for `rows` rows
};
inline So2Extents extents(const smrt::So2Batch& d, size_t rows) {
    const size_t N = (size_t)d.fo.n_pairs, L = d.fo.Lmax, T = d.fo.n_theta, NM = d.nmax, FS = (size_t)d.fo.F * d.fo.S;
    const size_t nslots = 2 + (d.interlayer ? L : 0);   // intralayer, substrate, one per layer with interlayer scattering
    return {NM, FS * L * T * NM * d.m_max * smrt::kSo2SubDoubles, N * 28 * T, extents(d.fo).layer_backscatter,
            rows * L, rows * L * 2 * NM, rows * L * T * nslots * 4};
}

// ---- successive order, passive and active ------------------------------------------------------------------------------------
inline smrt::SoBatch successive_order(const smrt_batch* b, int32_t n_iteration_max, double relative_tolerance, long long n_pairs) {
    smrt::SoBatch d{};
    shape(d, b, b->n_frequencies, b->n_theta, b->substrate_kind, n_pairs);
    d.nmax = b->n_max_stream;
    d.n_iter = n_iteration_max; d.rj = b->rayleigh_jeans ? 1 : 0; d.nsamp = smrt::azimuth_samples(b->m_max);
    d.rtol = relative_tolerance;
    return d;
}
struct SoExtents {
    size_t theta, sub_T, gl_mu;
    size_t stage, nsub, nstream, vec, srcterm, ws_off, out, status, layer_out, streams, maxrad, orders;
    size_t wt_pair;     // doubles of the transposed weighted phase matrices of one pair (the chunk buffer holds them per chunk)
    size_t lds_sweep;   // bytes
};
inline SoExtents extents(const smrt::SoBatch& d) {
    const size_t N = (size_t)d.n_pairs, L = d.Lmax, T = d.n_theta, NM = d.nmax, NO = d.n_iter, Dh = 2 * NM, Dp = smrt::so_dp(d.nmax);
    return {T, d.sub_kind == SMRT_SUBSTRATE_NONE ? 0 : (size_t)d.S, NM,
            (size_t)smrt::SO_ROWS * L * N, N * L, N * L, N * L * smrt::SO_VECS * Dh, N * L, N, N * (NO + 1) * 2 * T, N, N * L * 5,
            N * (1 + NM), N * NO, N,
            L * Dp * Dp, (size_t)smrt::so_lds_doubles(d.nmax, d.n_theta) * sizeof(double)};
}

inline smrt::SoaBatch successive_order_active(const smrt_batch* b, int32_t n_iteration_max, double relative_tolerance,
                                              int32_t n_theta_inc, int32_t incident_npol, int32_t m_max, long long n_pairs) {
    smrt::SoaBatch a{};
    a.so = successive_order(b, n_iteration_max, relative_tolerance, n_pairs);
    a.so.n_theta = n_theta_inc; a.so.rj = 0; a.so.nsamp = smrt::azimuth_samples(m_max);
    a.npi = incident_npol; a.m_max = m_max; a.Cmax = smrt::soa_max_columns(incident_npol, n_theta_inc, b->n_max_stream); a.phi = b->phi;
    return a;
}
struct SoaExtents {
    size_t theta, gl_mu;
    size_t stage, nsub, nstream, vec, air, ws_off, out, status, layer_out, streams, maxrad, orders, back, inc;
    size_t wt_pair;     // doubles: (m_max + 1) modes of Lmax matrices
    size_t lds_sweep;   // bytes
};
inline SoaExtents extents(const smrt::SoaBatch& a) {
    const smrt::SoBatch& d = a.so;
    const size_t N = (size_t)d.n_pairs, L = d.Lmax, T = d.n_theta, NM = d.nmax, NO = d.n_iter, Dh = 3 * NM, Dp = smrt::soa_dp(d.nmax);
    const size_t NP = a.m_max + 2, CM = a.Cmax;
    return {T, NM,
            (size_t)smrt::SO_ROWS * L * N, N * L, N * L, N * L * smrt::SOA_VECS * Dh, N * 2 * Dh, N, N * 9 * T * (NO + 1), N, N * L * 5,
            N * (1 + NM), N * NP * NO, N * NP, N * NP * NO * 3 * CM, N * (1 + NM),
            (size_t)(a.m_max + 1) * L * Dp * Dp, (size_t)smrt::soa_lds_doubles(d.nmax) * sizeof(double)};
}

// ---- multi-Fresnel -----------------------------------------------------------------------------------------------------------
inline smrt::MfBatch multifresnel(const smrt_batch* b, const double* mu, double prune_deep_snowpack, int32_t prune_none,
                                  long long n_pairs) {
    smrt::MfBatch d{};
    shape(d, b, b->n_frequencies, b->n_theta, b->substrate_kind, n_pairs);
    d.prune = prune_none ? INFINITY : prune_deep_snowpack;
    for (int t = 1; t < b->n_theta; ++t) if (mu[t] > mu[d.steepest]) d.steepest = t;
    return d;
}
struct MfExtents { size_t mu, sub_T, stage, out, status, layers_used, tau_snowpack, layer_out; };
inline MfExtents extents(const smrt::MfBatch& d) {
    const size_t N = (size_t)d.n_pairs, L = d.Lmax, T = d.n_theta;
    return {T, (size_t)d.S, (size_t)smrt::MF_ROWS * (L + 1) * N, N * 2 * T, N * T, N, N, N * L * 5};
}

// ---- nadir altimetry: LRM, and SAR on the LRM part it embeds -----------------------------------------------------------------
// the first-order batch of the layer kernel both solvers share: one angle, no substrate
inline smrt::FoBatch altimetry_layers(const smrt_batch* b, int n_frequencies, long long n_pairs) {
    smrt::FoBatch d{};
    shape(d, b, n_frequencies, 1, SMRT_SUBSTRATE_NONE, n_pairs);
    return d;
}
// ... and the range window
inline void altimetry_window(smrt::LrmBatch& d, int ngate, int oversampling, int return_oversampled) {
    d.ngate = ngate; d.os = oversampling; d.N = ngate * oversampling;
    d.oversampled = return_oversampled ? 1 : 0;
    d.n_out = d.oversampled ? d.N : d.ngate;
}

inline int lrm_rows(const smrt_lrm_params* p) { return p->n_mu > 1 ? 2 * p->n_mu + 1 : p->return_contributions ? 3 : 1; }
inline int lrm_out_rows(const smrt_lrm_params* p) { return p->return_contributions ? 3 : p->skip_pfs_convolution ? lrm_rows(p) : 1; }

inline smrt::LrmBatch nadir_lrm_altimetry(const smrt_batch* b, const smrt_lrm_params* p, long long n_pairs) {
    smrt::LrmBatch d{};
    d.fo = altimetry_layers(b, b->n_frequencies, n_pairs);
    altimetry_window(d, p->ngate, p->oversampling, p->return_oversampled);
    d.n_mu = p->n_mu; d.shift = p->shift;
    d.contributions = p->return_contributions ? 1 : 0; d.skip_pfs = p->skip_pfs_convolution ? 1 : 0;
    d.rows = lrm_rows(p); d.out_rows = lrm_out_rows(p);
    d.altitude = p->altitude; d.bandwidth = p->pulse_bandwidth; d.gain = p->antenna_gain; d.gamma = p->gamma;
    d.off_nadir = p->off_nadir_angle; d.nominal_gate = p->nominal_gate; d.pulse_sigma = p->pulse_sigma;
    return d;
}
struct LrmExtents {
    size_t t_inc, per_snowpack, itf;   // per_snowpack: sigma_surface, surface_slope
    size_t stage, bs, prefix, vsd, out, z_gate, status, layer_out;
    size_t lds_vertical, lds_waveform;   // bytes
};
inline LrmExtents extents(const smrt::LrmBatch& d) {
    const size_t N = (size_t)d.fo.n_pairs, L = d.fo.Lmax, FS = (size_t)d.fo.F * d.fo.S;
    const FoExtents fo = extents(d.fo);
    return {(size_t)d.n_mu, (size_t)d.fo.S, FS * (L + 1) * (1 + d.n_mu),
            fo.stage, L * N, N * smrt::LRM_PREFIX_ROWS * (L + 1), N * d.rows * d.N, N * d.out_rows * d.n_out, N * d.n_out, N, fo.layer_out,
            smrt::lrm_vertical_lds_bytes(d.N, d.fo.Lmax), smrt::lrm_waveform_lds_bytes(d.N, d.n_mu)};
}

inline smrt::SarBatch nadir_sar_altimetry(const smrt_batch* b, const smrt_sar_params* p, long long n_pairs) {
    smrt::SarBatch d{};
    smrt::LrmBatch& lb = d.lrm;
    lb.fo = altimetry_layers(b, 1, n_pairs);
    altimetry_window(lb, p->ngate, p->oversampling_time, p->return_oversampled);
    lb.n_mu = 1; lb.rows = 1; lb.out_rows = 1; lb.sar = 1;
    lb.altitude = p->altitude; lb.bandwidth = p->pulse_bandwidth; lb.nominal_gate = p->nominal_gate;
    d.ndoppler = p->ndoppler; d.osd = p->oversampling_doppler; d.ND = p->ndoppler * p->oversampling_doppler;
    d.out_rows = p->n_rows; d.n_tab = p->n_tables;
    d.n_t = lb.n_out; d.n_d = lb.oversampled ? d.ND : d.ndoppler;
    d.prf = p->pulse_repetition_frequency; d.wavelength = p->wavelength; d.velocity = p->velocity; d.alpha = p->alpha;
    d.pitch = p->pitch_angle; d.roll = p->roll_angle; d.sigma_p = p->sigma_p; d.theta_lim = p->theta_lim;
    d.gamma_x = p->gamma_x; d.gamma_y = p->gamma_y; d.l_gamma = p->l_gamma; d.lz = p->lz; d.pu = p->pu; d.nu_coherent = p->nu_coherent;
    if (p->delay_doppler_model == SMRT_SAR_HALIMI14)
        smrt::sar_h14_setup(d, p->slant_range_correction ? 1 : 0, p->delay_window_widening, p->h14_pu, p->h14_gamma, p->burst_duration);
    return d;
}
struct SarExtents {
    LrmExtents lrm;   // (lrm.out, lrm.t_inc and the waveform's LDS are not used; lrm.itf is counted below)
    size_t tab_sigma, tab_index, boundary_values, row_map;
    size_t tables, h14_doppler, h14_kernel, echo, out;   // the two h14 buffers: 0 with Dinardo18
    size_t lds_combine, lds_h14_doppler, lds_h14_kernel, lds_h14_delay;   // bytes
};
inline SarExtents extents(const smrt::SarBatch& d) {
    const size_t N = (size_t)d.lrm.fo.n_pairs, S = d.lrm.fo.S, L = d.lrm.fo.Lmax, NT = d.n_tab, ND = d.ND;
    const bool h14 = d.model == smrt::kSarHalimi14;
    return {extents(d.lrm),
            NT, S, S * (L + 1) * smrt::SAR_BV, S * (2 * (L + 1) + 2),
            NT * (h14 ? 1 : 2) * d.lrm.N * ND, h14 ? ND * d.N_wide : 0, h14 ? NT * d.M : 0, N * (L + 1) * smrt::SAR_ECHO,
            N * d.out_rows * d.n_t * d.n_d,
            h14 ? smrt::sar_h14_combine_lds_bytes(d.lrm.N, d.osd) : smrt::sar_combine_lds_bytes(d.lrm.N, d.osd),
            smrt::sar_h14_doppler_lds_bytes(d.ND), h14 ? smrt::sar_h14_kernel_lds_bytes(d.M) : 0,
            h14 ? smrt::sar_h14_delay_lds_bytes(d.N_wide, d.M) : 0};
}

}  // namespace solver_describe
