// What each solver beside DORT refuses of a batch before any device work: the message, or null when the batch is taken.
// Pure host code (the CPU tests reach it through tests/hostemu/solver_refusals_host.cpp).  The checks all of them make are in
// dort_host_common.hpp (smrt_host::refuse_*); the order of the checks is part of the interface: callers match on the
// messages, and an input that fails two checks has always been answered with the first.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "dort_host_common.hpp"
#include "nadir_lrm_altimetry_kernel.hpp"   // lrm_vertical_lds_bytes, lrm_waveform_lds_bytes
#include "nadir_sar_altimetry_kernel.hpp"   // sar_combine_lds_bytes
#include "second_order_kernel.hpp"          // kSo2MaxModes
#include "successive_order_kernel.hpp"      // kSoMaxStream

namespace solver_refusals {
using namespace smrt_host;

inline const char* first_order(const smrt_batch* b, const smrt_first_order_extras* x) {
    static const SolverAccepts accepts{true, true, 0, nullptr, nullptr, SMRT_SUBSTRATE_REFLECTOR,
                                       "substrate_kind must be none, flat or reflector: any other substrate travels in smrt_first_order_extras", false};
    const char* why = refuse_empty(b);
    if (why) return why;
    if (b->n_theta <= 0) return "n_theta must be positive";
    if (b->mode != SMRT_MODE_ACTIVE) return "the iterative first-order solver needs an active sensor";
    if ((why = refuse_inputs(b, accepts))) return why;
    // layers evaluated by the caller bring their scalars
    bool host_scalars = !b->layer_kind && b->emmodel >= SMRT_EM_HOST && b->emmodel != SMRT_EM_IBA_INVERTED;
    bool iba_host = !b->layer_kind && b->emmodel == SMRT_EM_IBA_HOST;
    for (int s = 0; b->layer_kind && s < b->n_snowpacks; ++s)
        for (int l = 0; l < b->n_layers[s]; ++l) {
            const int em = b->layer_kind[(long long)s * b->n_layers_max + l] & 15;
            if (em == SMRT_EM_HOST || em == SMRT_EM_IBA_HOST || em == SMRT_EM_RAYLEIGH_HOST) host_scalars = true;
            if (em == SMRT_EM_IBA_HOST) iba_host = true;
        }
    if (host_scalars && !b->host_layer) return "layers evaluated by the caller need host_layer";
    if (iba_host && !b->host_iba_coeff) return "layers of kind SMRT_EM_IBA_HOST need host_iba_coeff";
    if ((why = refuse_substrate(b, accepts))) return why;
    if (x && x->host_interface_slot) {
        if (x->n_interface_slots < 1 || !x->host_interface_values) return "host_interface_slot needs host_interface_values and n_interface_slots >= 1";
        const long long n = (long long)b->n_frequencies * b->n_snowpacks * (b->n_layers_max + 1);
        for (long long i = 0; i < n; ++i)
            if (x->host_interface_slot[i] < -1 || x->host_interface_slot[i] >= x->n_interface_slots) return "host_interface_slot entry out of range";
    }
    return nullptr;
}

// What the second-order solver adds in front of first_order(), which sees the batch next (before n_layers has been
// checked: the layer loop stays inside the array)
inline const char* second_order(const smrt_batch* b) {
    if (!b) return "null batch";
    if (b->n_max_stream < 2 || b->n_max_stream > 1024) return "n_max_stream must be 2 to 1024";
    if (b->m_max < 1 || b->m_max > smrt::kSo2MaxModes) return "m_max must be 1 to 8";
    if (!b->layer_kind && b->emmodel == SMRT_EM_HOST) return "the iterative second-order solver has no route for emmodels evaluated by the caller (SMRT_EM_HOST)";
    for (int s = 0; b->layer_kind && b->n_layers && s < b->n_snowpacks; ++s)
        for (int l = 0; l < b->n_layers[s] && l < b->n_layers_max; ++l)
            if ((b->layer_kind[(long long)s * b->n_layers_max + l] & 15) == SMRT_EM_HOST)
                return "the iterative second-order solver has no route for emmodels evaluated by the caller (SMRT_EM_HOST)";
    return nullptr;
}

inline const char* successive_order(const smrt_batch* b, int32_t n_iter, double rtol) {
    static const SolverAccepts accepts{true, true, kHostEmmodels, "the successive_order solver has no route for emmodels evaluated on the host", nullptr,
                                       SMRT_SUBSTRATE_REFLECTOR, "the successive_order solver takes no substrate, a flat one or a reflector", false,
                                       true};   // (and the rough soils, which are diagonal per stream like the flat one)
    const char* why = refuse_empty(b);
    if (why) return why;
    if (b->n_theta <= 0) return "n_theta must be positive";
    if (b->mode != SMRT_MODE_PASSIVE) return "the successive_order solver needs a passive sensor";
    if (n_iter < 1) return "n_iteration_max must be at least 1";
    if (!(rtol >= 0.0)) return "relative_tolerance must be non-negative";
    if (b->n_max_stream < 2 || b->n_max_stream > smrt::kSoMaxStream) return "the successive_order solver takes 2 to 64 streams";
    if (b->m_max < 0) return "m_max must be non-negative";
    if ((why = refuse_inputs(b, accepts)) || (why = refuse_substrate(b, accepts))) return why;
    if (b->host_interface_slot) return "the successive_order solver takes flat interfaces only";
    if (b->atm_tb_down || b->atm_tb_up || b->atm_transmittance) return "the successive_order solver can not handle atmosphere yet.";
    if (b->process_coherent_layers) return "the successive_order solver does not process coherent layers";
    return nullptr;
}

inline const char* successive_order_active(const smrt_batch* b, int32_t n_iter, double rtol, int32_t n_theta_inc, const double* theta_inc,
                                           int32_t incident_npol, int32_t m_max) {
    const SolverAccepts accepts{false, true, kHostEmmodels, "the successive_order_backscatter solver has no route for emmodels evaluated on the host",
                                m_max > 2 ? "the Rayleigh-family emmodels have azimuth modes 0 to 2 only: m_max must be at most 2" : nullptr, SMRT_SUBSTRATE_FLAT,
                                "the successive_order_backscatter solver takes no substrate or a flat one (a reflector has no third Stokes component)", false};
    const char* why = refuse_empty(b);
    if (why) return why;
    if (n_theta_inc <= 0 || !theta_inc) return "n_theta_inc must be positive";
    if (b->mode != SMRT_MODE_ACTIVE) return "the successive_order_backscatter solver needs an active sensor";
    if (n_iter < 1) return "n_iteration_max must be at least 1";
    if (!(rtol >= 0.0)) return "relative_tolerance must be non-negative";
    if (incident_npol < 1 || incident_npol > 3) return "incident_npol must be 1 (V), 2 (VH) or 3 (VHU)";
    if (b->n_max_stream < 2 || b->n_max_stream > smrt::kSoMaxStream) return "the successive_order_backscatter solver takes 2 to 64 streams";
    if (m_max < 0 || m_max > 64) return "m_max must be 0 to 64";
    if ((why = refuse_inputs(b, accepts)) || (why = refuse_substrate(b, accepts))) return why;
    if (b->host_interface_slot) return "the successive_order_backscatter solver takes flat interfaces only";
    if (b->process_coherent_layers) return "the successive_order_backscatter solver does not process coherent layers";
    return nullptr;
}

inline const char* multifresnel(const smrt_batch* b, const double* mu, double prune, int32_t prune_none) {
    // (every emmodel code but the five with a device implementation, the codes no emmodel has included)
    constexpr unsigned on_device = 1u << SMRT_EM_IBA | 1u << SMRT_EM_DMRT_QCA_SHORTRANGE | 1u << SMRT_EM_DMRT_QCACP_SHORTRANGE |
                                   1u << SMRT_EM_NONSCATTERING | 1u << SMRT_EM_IBA_INVERTED;
    static const SolverAccepts accepts{false, true, ~on_device, "the multi-Fresnel thermal emission solver needs emmodels with a device implementation", nullptr,
                                       SMRT_SUBSTRATE_FLAT, "the multi-Fresnel thermal emission solver takes no substrate or a Flat one", true};
    const char* why = refuse_empty(b);
    if (why) return why;
    if (b->n_theta <= 0 || !mu) return "the sensor cosines are missing";
    if (b->mode != SMRT_MODE_PASSIVE) return "the multi-Fresnel thermal emission solver needs a passive sensor";
    if (b->atm_tb_down || b->atm_tb_up || b->atm_transmittance) return "the multi-Fresnel thermal emission solver can not handle atmosphere";
    if (b->host_interface_slot) return "the multi-Fresnel thermal emission solver takes Flat interfaces only";
    if (b->host_layer || b->host_phase || b->host_iba_coeff) return accepts.emmodel_refusal;
    if (b->process_coherent_layers) return "process_coherent_layers is not available in the multi-Fresnel thermal emission solver";
    if ((why = refuse_inputs(b, accepts)) || (why = refuse_substrate(b, accepts))) return why;
    if (!prune_none && std::isnan(prune)) return "prune_deep_snowpack is not a number";
    return nullptr;
}

constexpr size_t kLrmLdsLimit = 160 * 1024 - 64;   // dynamic LDS of a workgroup: the 160 KB of a CU less the kernels' static bytes

inline const char* nadir_lrm_altimetry(const smrt_batch* b, const smrt_lrm_params* p) {
    static const SolverAccepts accepts{false, false, 0, nullptr, nullptr, 0, nullptr, false};   // (any mode; the substrate is not read)
    if (!b || !p) return "null batch or parameters";
    const char* why = refuse_empty(b);
    if (why) return why;
    if (b->atm_tb_down || b->atm_tb_up || b->atm_transmittance) return "the nadir LRM altimetry solver can not handle atmosphere";
    if (b->host_phase) return "the nadir LRM altimetry solver has no route for phase matrices evaluated on the host";
    if (b->process_coherent_layers) return "process_coherent_layers is not available in the nadir LRM altimetry solver";
    if ((why = refuse_inputs(b, accepts))) return why;
    if (p->ngate < 1 || p->oversampling < 1) return "ngate and oversampling_time must be positive";
    if ((long long)p->ngate * p->oversampling > (1 << 20)) return "ngate x oversampling_time is too large";
    if (p->n_mu < 1 || (p->n_mu > 1 && !p->t_inc)) return "the times of the incidence samples are missing";
    if (p->n_mu > 1 && p->skip_pfs_convolution) return "skip_pfs_convolution needs theta_inc_sampling = 1";
    if (!(p->altitude > 0.0) || !(p->pulse_bandwidth > 0.0) || !(p->gamma > 0.0) || !(p->pulse_sigma > 0.0)) return "invalid sensor parameters";
    if (p->n_mu == 1 && !p->skip_pfs_convolution && (p->shift < 1 || p->shift >= p->ngate * p->oversampling))
        return "the nominal gate must lie inside the gate window, after its first sub-gate";
    if (p->n_mu > 1 && p->sigma_surface) return "sigma_surface needs theta_inc_sampling = 1";
    const size_t a = smrt::lrm_vertical_lds_bytes(p->ngate * p->oversampling, b->n_layers_max);
    const size_t c = smrt::lrm_waveform_lds_bytes(p->ngate * p->oversampling, p->n_mu);
    if (a > kLrmLdsLimit || c > kLrmLdsLimit) return "ngate x oversampling_time (and the layers) do not fit the local data share";
    return nullptr;
}

constexpr size_t kSarOutputBudget = (size_t)2 << 30;   // bytes of the maps of one launch (the caller splits the pairs)

inline const char* nadir_sar_altimetry(const smrt_batch* b, const smrt_sar_params* p) {
    static const SolverAccepts accepts{false, false, 0, nullptr, nullptr, 0, nullptr, false};   // (any mode; the substrate is not read)
    if (!b || !p) return "null batch or parameters";
    const char* why = refuse_empty(b);
    if (why) return why;
    if (b->n_frequencies != 1) return "the nadir SAR altimetry solver takes one frequency per batch (the sensor constants depend on it)";
    if (b->atm_tb_down || b->atm_tb_up || b->atm_transmittance) return "the nadir SAR altimetry solver can not handle atmosphere";
    if (b->host_phase) return "the nadir SAR altimetry solver has no route for phase matrices evaluated on the host";
    if (b->process_coherent_layers) return "process_coherent_layers is not available in the nadir SAR altimetry solver";
    if ((why = refuse_inputs(b, accepts))) return why;
    if (p->ngate < 1 || p->oversampling_time < 1 || p->oversampling_doppler < 1) return "ngate and the oversampling factors must be positive";
    if (p->ndoppler < 2 || p->ndoppler % 2) return "ndoppler must be even and positive (the reference's Doppler axis has another length than its map otherwise)";
    if ((long long)p->ngate * p->oversampling_time > (1 << 20) || (long long)p->ndoppler * p->oversampling_doppler > (1 << 20))
        return "the oversampled map is too large";
    if (!(p->altitude > 0.0) || !(p->pulse_bandwidth > 0.0) || !(p->velocity > 0.0) || !(p->pulse_repetition_frequency > 0.0) ||
        !(p->sigma_p > 0.0) || !(p->theta_lim > 0.0) || !(p->gamma_y > 0.0) || !(p->l_gamma > 0.0) || !(p->lz > 0.0))
        return "invalid sensor parameters";
    if (!p->table_sigma || !p->table_index || !p->boundary_values || !p->row_map || p->n_tables < 1) return "the tables, the boundary values or the row map are missing";
    if (p->n_rows < 1) return "n_rows must be positive";
    if (p->delay_doppler_model != SMRT_SAR_DINARDO18 && p->delay_doppler_model != SMRT_SAR_HALIMI14)
        return "unknown delay_doppler_model: the nadir SAR altimetry solver has Dinardo18 (0) and Halimi14 (1)";
    if (p->delay_doppler_model == SMRT_SAR_HALIMI14) {
        if (p->delay_window_widening < 1) return "delay_window_widening must be at least 1";
        if (p->ngate * p->oversampling_time < 2) return "Halimi14 needs at least two delay samples (its time point target response has 2 (N / 2) - 1)";
        if (!(p->h14_pu > 0.0) || !(p->h14_gamma > 0.0) || !(p->burst_duration > 0.0)) return "invalid sensor parameters";
        const long long n_wide = (long long)p->ngate * p->oversampling_time * p->delay_window_widening;
        const int nd = p->ndoppler * p->oversampling_doppler, m = 2 * (p->ngate * p->oversampling_time / 2) - 1;
        if (n_wide > (1 << 20) || smrt::sar_h14_doppler_lds_bytes(nd) > kLrmLdsLimit || smrt::sar_h14_delay_lds_bytes((int)n_wide, m) > kLrmLdsLimit)
            return "the widened delay window or the Doppler axis of Halimi14 do not fit the local data share";
    }
    for (int t = 0; t < p->n_tables; ++t)
        if (!(p->table_sigma[t] >= 0.0)) return "sigma_surface must be non-negative";
    const int sources = 2 * (b->n_layers_max + 1) + 2;
    for (int s = 0; s < b->n_snowpacks; ++s) {
        if (p->table_index[s] < 0 || p->table_index[s] >= p->n_tables) return "table_index entry out of range";
        for (int k = 0; k < sources; ++k)
            if (p->row_map[(long long)s * sources + k] < -1 || p->row_map[(long long)s * sources + k] >= p->n_rows) return "row_map entry out of range";
    }
    const size_t a = smrt::lrm_vertical_lds_bytes(p->ngate * p->oversampling_time, b->n_layers_max);
    const size_t c = smrt::sar_combine_lds_bytes(p->ngate * p->oversampling_time, p->oversampling_doppler);
    if (a > kLrmLdsLimit || c > kLrmLdsLimit) return "ngate x oversampling_time x oversampling_doppler (and the layers) do not fit the local data share";
    return nullptr;
}

}  // namespace solver_refusals
