// Host-side helpers shared by the HIP library (dort_hip.hip) and the emulator build used by the CPU tests.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../include/smrt_dort.h"

// Jacobi thresholds of the pipelines in passive mode (squared cosines; the kernels take them as run-time parameters):
// rotations below SKIP are not applied, a sweep without a rotation above EXIT is the last one.  Active mode keeps
// 1e-30 / 1e-22 (dort_jacobi_kernel.hpp).  Two sets:
//  * the pipelines that solve with the eigenvector matrices as they come (two-slot / global-workspace / big finish kernels):
//    1e-24 / 1e-14 since round 4.  The 1e-22 / 1e-12 of round 3 (2e-8 K on ordinary snow) were 4.4e-5 K off on a wet,
//    weakly scattering snowpack of the randomised sweep (tools/stress_vs_oracle.py 71 wetmicro, 40 streams: nearly
//    degenerate singular values again -- ADVICE r3 had asked for exactly this check); 1e-24 / 1e-14: 1.4e-9 K on that
//    sweep for 1.2 % of the configs[2]-shape step, 1e-26 / 1e-15: 1.4e-10 K for 2.1 %;
//  * the register-resident finish kernel uses the orthogonality itself (the inverses of the eigenvector matrices are their
//    transposes): with 1e-22 / 1e-12 it is at 1.6e-8 K on the headline batch but loses up to 2.4e-4 K on weakly
//    scattering media (1.4 GHz: nearly degenerate singular values) -- tools/stress_reg_extremes.py, 860 hard pairs:
//    1e-24 / 1e-14 -> 2.6e-6 K, 1e-26 / 1e-15 -> 1.3e-7 K (+1.1 ms per headline step), 1e-28 / 1e-16 -> 1.9e-8 K (+1.5 ms).
//    The requirement is 1e-6 K.
#ifndef SMRT_JACOBI_PASSIVE_SKIP_COS2
#define SMRT_JACOBI_PASSIVE_SKIP_COS2 1e-24
#endif
#ifndef SMRT_JACOBI_PASSIVE_EXIT_COS2
#define SMRT_JACOBI_PASSIVE_EXIT_COS2 1e-14
#endif
#ifndef SMRT_JACOBI_REG_SKIP_COS2
#define SMRT_JACOBI_REG_SKIP_COS2 1e-26
#endif
#ifndef SMRT_JACOBI_REG_EXIT_COS2
#define SMRT_JACOBI_REG_EXIT_COS2 1e-15
#endif

namespace smrt_host {

// The transfers of smrt_dort_gather as data, so that the offset / count arithmetic can be tested with any number of ranks
// on a machine with one GPU or none (tests/test_multirank_cpu.py): on the root one receive per other rank that has rows
// (the rows of rank r land at row offset sum(counts[0..r)) of the gathered buffer, own rows copied to own_offset), on
// every other rank one send of its counts[rank] rows (none when it has no rows).  Returns the number of ops, -1 on
// invalid arguments.
inline int gather_plan(int world, int root, int rank, const int64_t* counts, smrt_gather_op* ops, int capacity,
                       int64_t* own_offset_rows, int64_t* total_rows) {
    if (world < 1 || root < 0 || root >= world || rank < 0 || rank >= world || !counts) return -1;
    int64_t total = 0, own = 0;
    for (int r = 0; r < world; ++r) {
        if (counts[r] < 0) return -1;
        if (r == rank) own = total;
        total += counts[r];
    }
    if (own_offset_rows) *own_offset_rows = (rank == root) ? own : 0;
    if (total_rows) *total_rows = total;
    int n = 0;
    if (rank != root) {
        if (counts[rank] > 0) {
            if (ops && n < capacity) { ops[n].peer = root; ops[n].offset_rows = 0; ops[n].rows = counts[rank]; }
            ++n;
        }
        return n;
    }
    int64_t off = 0;
    for (int r = 0; r < world; ++r) {
        if (r != root && counts[r] > 0) {
            if (ops && n < capacity) { ops[n].peer = r; ops[n].offset_rows = off; ops[n].rows = counts[r]; }
            ++n;
        }
        off += counts[r];
    }
    return n;
}

// Positive nodes (descending) and weights of the Gauss-Legendre rule of order 2n, by Newton iteration on the
// three-term recurrence (what scipy.special.roots_legendre provides to smrt/rtsolver/streams.py:300-313).
inline void gauss_legendre_positive(int n, double* mu, double* weight) {
    const int m = 2 * n;
    for (int i = 0; i < n; ++i) {
        double x = std::cos(M_PI * (i + 0.75) / (m + 0.5));  // i-th largest root
        double dp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p0 = 1.0, p1 = x;
            for (int k = 2; k <= m; ++k) {
                const double pk = ((2.0 * k - 1.0) * x * p1 - (k - 1.0) * p0) / k;
                p0 = p1;
                p1 = pk;
            }
            dp = m * (x * p1 - p0) / (x * x - 1.0);
            const double dx = p1 / dp;
            x -= dx;
            if (std::fabs(dx) < 1e-16) break;
        }
        // final derivative at the converged node
        double p0 = 1.0, p1 = x;
        for (int k = 2; k <= m; ++k) {
            const double pk = ((2.0 * k - 1.0) * x * p1 - (k - 1.0) * p0) / k;
            p0 = p1;
            p1 = pk;
        }
        (void)dp;
        mu[i] = x;
        if (weight) weight[i] = 2.0 * (1.0 - x * x) / ((double)m * (double)m * p0 * p0);  // 2(1-x^2)/(m P_{m-1}(x))^2
    }
}

inline int out_stride(const smrt_batch* b) {
    return (b->mode == SMRT_MODE_PASSIVE) ? 2 * b->n_theta : 9 * b->n_theta;
}

// The rough soils the device evaluates per stream in passive mode: substrate_p1 / substrate_p2 carry [S][2] parameters behind
// their [F][S] permittivities (smrt_dort.h).
inline bool is_soil_substrate(int kind) { return kind >= SMRT_SUBSTRATE_SOIL_WEGMULLER && kind <= SMRT_SUBSTRATE_ROUGH_CHOUDHURY; }
// doubles in substrate_p1 (and in substrate_p2) of a batch with a substrate of this kind
inline size_t substrate_array_doubles(const smrt_batch* b) {
    return (size_t)b->n_frequencies * b->n_snowpacks + (is_soil_substrate(b->substrate_kind) ? 2 * (size_t)b->n_snowpacks : 0);
}

// Rough boundaries evaluated on the device: is the substrate of the batch one of them (entry n_layers of the first snowpack;
// validate() holds the others to the same answer)?
inline bool rough_substrate(const smrt_batch* b) {
    return b->rough_kind && b->n_layers && b->rough_kind[b->n_layers[0]] != SMRT_ROUGH_NONE;
}

inline const char* refuse_rough(const smrt_batch* b) {
    if (!b->rough_kind) return nullptr;
    if (!b->rough_params) return "rough_kind needs rough_params";
    if (b->host_interface_slot || b->substrate_kind == SMRT_SUBSTRATE_HOST)
        return "rough_kind cannot be combined with host_interface_slot or SMRT_SUBSTRATE_HOST: the rough boundaries of a batch take one route";
    if (b->process_coherent_layers)
        return "rough_kind cannot be combined with process_coherent_layers: hand the rough boundaries over as host_interface / SMRT_SUBSTRATE_HOST";
    if (b->mode == SMRT_MODE_ACTIVE && b->m_max > SMRT_ROUGH_M_MAX)
        return "rough_kind: m_max beyond SMRT_ROUGH_M_MAX, the largest the rough-boundary kernels are instantiated for";
    const bool sub = rough_substrate(b);
    if (sub && b->substrate_kind != SMRT_SUBSTRATE_FLAT)
        return "a rough substrate on the device needs substrate_kind = SMRT_SUBSTRATE_FLAT (its permittivity in substrate_p1 / substrate_p2)";
    const long long W = (long long)b->n_layers_max + 1;
    for (int s = 0; s < b->n_snowpacks; ++s) {
        if (b->n_layers[s] < 1 || b->n_layers[s] > b->n_layers_max) return "n_layers out of range";
        for (int l = 0; l <= b->n_layers[s]; ++l) {
            const int k = b->rough_kind[s * W + l];
            if (k < SMRT_ROUGH_NONE || k > SMRT_ROUGH_IEM_FUNG92) return "unknown rough_kind entry";
        }
        if ((b->rough_kind[s * W + b->n_layers[s]] != SMRT_ROUGH_NONE) != sub)
            return "rough_kind: the substrates of a batch are rough on the device for every snowpack or for none";
    }
    return nullptr;
}

inline const char* validate(const smrt_batch* b) {
    if (!b) return "null batch";
    if (b->n_snowpacks <= 0 || b->n_frequencies <= 0 || b->n_layers_max <= 0) return "empty batch";
    if (b->n_theta <= 0) return "n_theta must be positive";
    if (b->n_max_stream < 2) return "n_max_stream must be >= 2";
    if (b->emmodel < SMRT_EM_IBA || b->emmodel > SMRT_EM_RAYLEIGH_HOST) return "unknown emmodel";
    bool host_layers = (!b->layer_kind && b->emmodel == SMRT_EM_HOST);
    bool scalar_layers = (!b->layer_kind && b->emmodel == SMRT_EM_IBA_HOST);
    bool rayleigh_layers = (!b->layer_kind && b->emmodel == SMRT_EM_RAYLEIGH_HOST);
    if (b->microstructure < SMRT_MS_EXPONENTIAL || b->microstructure > SMRT_MS_TEUBNER_STREY)
        return "unknown microstructure";
    if (!b->layer_kind && (b->emmodel == SMRT_EM_DMRT_QCA_SHORTRANGE || b->emmodel == SMRT_EM_DMRT_QCACP_SHORTRANGE) &&
        b->microstructure != SMRT_MS_STICKY_HARD_SPHERES)
        return "the dmrt short-range emmodels are only compatible with sticky_hard_spheres";
    if (b->layer_kind && b->n_layers)
        for (int s = 0; s < b->n_snowpacks; ++s)
            for (int l = 0; l < b->n_layers[s]; ++l) {
                const int k = b->layer_kind[(long long)s * b->n_layers_max + l], em = k & 15, ms = k >> 4;
                if (em < SMRT_EM_IBA || em > SMRT_EM_RAYLEIGH_HOST || ms < SMRT_MS_EXPONENTIAL || ms > SMRT_MS_TEUBNER_STREY_COMPLEX_K)
                    return "invalid layer_kind entry";
                if (ms >= SMRT_MS_EXPONENTIAL_COMPLEX_K && (em != SMRT_EM_IBA_HOST || b->mode != SMRT_MODE_PASSIVE))
                    return "SMRT_MS_*_COMPLEX_K go with SMRT_EM_IBA_HOST layers in passive mode only";
                if (ms == SMRT_MS_STICKY_HARD_SPHERES_COMPLEX_K || ms == SMRT_MS_INDEPENDENT_SPHERE_COMPLEX_K)
                    return "the sphere models have no complex-wavenumber form on the device (exponential and Teubner-Strey do)";
                if (em == SMRT_EM_HOST) host_layers = true;
                if (em == SMRT_EM_IBA_HOST) scalar_layers = true;
                if (em == SMRT_EM_RAYLEIGH_HOST) rayleigh_layers = true;
                if ((em == SMRT_EM_DMRT_QCA_SHORTRANGE || em == SMRT_EM_DMRT_QCACP_SHORTRANGE) && ms != SMRT_MS_STICKY_HARD_SPHERES)
                    return "the dmrt short-range emmodels are only compatible with sticky_hard_spheres";
            }
    if (host_layers && (!b->host_layer || !b->host_streams || !b->host_phase))
        return "layers of kind SMRT_EM_HOST need host_layer, host_streams and host_phase";
    if (scalar_layers && (!b->host_layer || !b->host_iba_coeff))
        return "layers of kind SMRT_EM_IBA_HOST need host_layer and host_iba_coeff";
    if (rayleigh_layers && !b->host_layer) return "layers of kind SMRT_EM_RAYLEIGH_HOST need host_layer";
    if (b->mode != SMRT_MODE_PASSIVE && b->mode != SMRT_MODE_ACTIVE) return "unknown mode";
    if (!b->n_layers || !b->thickness || !b->frac_volume || !b->temperature || !b->micro_p1 || !b->frequency ||
        !b->theta)
        return "null input array";
    if ((b->microstructure == SMRT_MS_STICKY_HARD_SPHERES || b->layer_kind) && !b->micro_p2) return "stickiness array missing";
    if (b->substrate_kind < SMRT_SUBSTRATE_NONE || b->substrate_kind > SMRT_SUBSTRATE_ROUGH_CHOUDHURY) return "unknown substrate kind";
    if (b->substrate_kind == SMRT_SUBSTRATE_HOST) {
        if (!b->host_substrate || !b->host_substrate_coh) return "SMRT_SUBSTRATE_HOST needs host_substrate and host_substrate_coh";
        if (b->mode == SMRT_MODE_PASSIVE && !b->substrate_temperature) return "SMRT_SUBSTRATE_HOST in passive mode needs substrate_temperature";
    } else
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE && (!b->substrate_p1 || !b->substrate_p2 || !b->substrate_temperature))
        return "substrate arrays missing";
    if (b->substrate_kind == SMRT_SUBSTRATE_REFLECTOR && b->mode == SMRT_MODE_ACTIVE)
        return "the reflector substrate has no third Stokes component: passive mode only (smrt/substrate/reflector.py)";
    if (is_soil_substrate(b->substrate_kind) && b->mode == SMRT_MODE_ACTIVE)
        return "the Wegmuller, QNH and Choudhury substrates are evaluated on the device in passive mode only: hand them over as SMRT_SUBSTRATE_HOST in active mode";
    if (b->host_interface_slot) {
        if (!b->host_interface || !b->host_interface_coh || b->host_interface_slots < 1)
            return "host_interface_slot needs host_interface, host_interface_coh and host_interface_slots >= 1";
        const long long n = (long long)b->n_frequencies * b->n_snowpacks * b->n_layers_max;
        for (long long i = 0; i < n; ++i)
            if (b->host_interface_slot[i] < -1 || b->host_interface_slot[i] >= b->host_interface_slots) return "host_interface_slot entry out of range";
    }
    if ((b->atm_tb_down != nullptr) != (b->atm_tb_up != nullptr) || (b->atm_tb_down != nullptr) != (b->atm_transmittance != nullptr))
        return "atmosphere arrays must be given together";
    return refuse_rough(b);
}

// What the solvers beside DORT refuse alike (solver_refusals.hpp holds each solver's own checks, and calls these between
// them in the order its refusals have always had).  What a solver accepts of the batch:
struct SolverAccepts {
    bool theta;                      // b->theta is read: null is refused
    bool layer_emmodels;             // false: emmodel codes are not looked at (every one evaluates, or the solver checks them itself)
    unsigned emmodel_refused;        // bit e: emmodel code e (of the batch, or of a layer_kind entry) is refused ...
    const char* emmodel_refusal;     // ... with this message
    const char* dmrt_refusal;        // not null: refuses the DMRT short-range emmodels (after their microstructure check)
    int substrate_last;              // substrate kinds SMRT_SUBSTRATE_NONE .. substrate_last are taken ...
    const char* substrate_refusal;   // ... the others refused with this message
    bool substrate_temperature;      // a substrate needs substrate_temperature too
    bool soil_substrates = false;    // SMRT_SUBSTRATE_SOIL_WEGMULLER .. _ROUGH_CHOUDHURY are taken as well (they always need all three arrays)
};
constexpr unsigned kHostEmmodels = 1u << SMRT_EM_HOST | 1u << SMRT_EM_IBA_HOST | 1u << SMRT_EM_RAYLEIGH_HOST;

inline const char* refuse_empty(const smrt_batch* b) {
    if (!b) return "null batch";
    if (b->n_snowpacks <= 0 || b->n_frequencies <= 0 || b->n_layers_max <= 0) return "empty batch";
    return nullptr;
}

inline const char* refuse_emmodel(int em, int ms, const SolverAccepts& a) {
    if (a.emmodel_refused >> em & 1) return a.emmodel_refusal;
    if (em == SMRT_EM_DMRT_QCA_SHORTRANGE || em == SMRT_EM_DMRT_QCACP_SHORTRANGE) {
        if (ms != SMRT_MS_STICKY_HARD_SPHERES) return "the dmrt short-range emmodels are only compatible with sticky_hard_spheres";
        return a.dmrt_refusal;
    }
    return nullptr;
}

// the model codes, the input arrays, n_layers and the layer_kind entries (a non-empty batch)
inline const char* refuse_inputs(const smrt_batch* b, const SolverAccepts& a) {
    // (only DORT builds rough boundaries on the device: every other solver would take the interfaces for flat)
    if (b->rough_kind || b->rough_params) return "rough_kind / rough_params are read by the DORT solver only: this solver would take the boundaries for flat";
    if (b->emmodel < SMRT_EM_IBA || b->emmodel > SMRT_EM_RAYLEIGH_HOST) return "unknown emmodel";
    if (b->microstructure < SMRT_MS_EXPONENTIAL || b->microstructure > SMRT_MS_TEUBNER_STREY) return "unknown microstructure";
    if (!b->n_layers || !b->thickness || !b->frac_volume || !b->temperature || !b->micro_p1 || !b->frequency || (a.theta && !b->theta))
        return "null input array";
    if ((b->microstructure == SMRT_MS_STICKY_HARD_SPHERES || b->layer_kind) && !b->micro_p2) return "stickiness array missing";
    const char* why = (a.layer_emmodels && !b->layer_kind) ? refuse_emmodel(b->emmodel, b->microstructure, a) : nullptr;
    if (why) return why;
    for (int s = 0; s < b->n_snowpacks; ++s) {
        if (b->n_layers[s] < 1 || b->n_layers[s] > b->n_layers_max) return "n_layers out of range";
        for (int l = 0; b->layer_kind && l < b->n_layers[s]; ++l) {
            const int k = b->layer_kind[(long long)s * b->n_layers_max + l], em = k & 15, ms = k >> 4;
            if (ms < SMRT_MS_EXPONENTIAL || ms > SMRT_MS_TEUBNER_STREY) return "invalid layer_kind entry";
            if (!a.layer_emmodels) continue;
            if (em > SMRT_EM_RAYLEIGH_HOST && !(a.emmodel_refused >> em & 1)) return "invalid layer_kind entry";
            if ((why = refuse_emmodel(em, ms, a))) return why;
        }
    }
    return nullptr;
}

inline const char* refuse_substrate(const smrt_batch* b, const SolverAccepts& a) {
    const bool soil = is_soil_substrate(b->substrate_kind);
    if (b->substrate_kind < SMRT_SUBSTRATE_NONE || (soil ? !a.soil_substrates : b->substrate_kind > a.substrate_last)) return a.substrate_refusal;
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE && (!b->substrate_p1 || !b->substrate_p2 || ((a.substrate_temperature || soil) && !b->substrate_temperature)))
        return "substrate arrays missing";
    return nullptr;
}

// The pair list of an *_upload_pairs call: null means all `all` pairs (*n_pairs is set), otherwise every index must be one.
inline const char* refuse_pairs(const int64_t* pairs, int64_t* n_pairs, int64_t all) {
    if (!pairs) { *n_pairs = all; return nullptr; }
    if (*n_pairs <= 0) return "empty pair list";
    for (int64_t i = 0; i < *n_pairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= all) return "pair index out of bounds";
    return nullptr;
}

}  // namespace smrt_host
