// The device arithmetic of the nadir SAR altimetry solver (smrt_amd/csrc/nadir_sar_altimetry_kernel.hpp) compiled for the CPU with
// BOTH delay-Doppler models: what nadir_sar_altimetry_host.cpp does for Dinardo18, and the table stage and the map of Halimi et
// al. 2014 as smrt_sar_launch runs them.  A "workgroup" is one thread.  Built by tests/test_nadir_sar_altimetry_halimi14_cpu.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_sar_halimi14_host.so nadir_sar_altimetry_halimi14_host.cpp
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../smrt_amd/csrc/solver_refusals.hpp"
#include "../../include/smrt_dort.h"

using namespace smrt;

// Same batch, parameters and outputs as smrt_sar_run_pairs over every pair, without a context.  `table` (may be null) receives the
// first table of Halimi14 as the reference lays it out, [ngate x oversampling_time][ndoppler x oversampling_doppler].
// Returns 0, or -1 (refused).
extern "C" __attribute__((visibility("default")))
int32_t smrt_sar_host_run_table(const smrt_batch* b, const smrt_sar_params* p, double* out, int32_t* status, double* z_gate,
                                double* layer_out, double* vertical, double* echo, double* table) {
    if (!out || !status || !z_gate || !layer_out || !vertical || !echo) return -1;
    if (solver_refusals::nadir_sar_altimetry(b, p)) return -1;
    const long long NP = b->n_snowpacks;
    const int L = b->n_layers_max;
    const bool h14 = p->delay_doppler_model == SMRT_SAR_HALIMI14;
    std::vector<int> nl(b->n_layers, b->n_layers + b->n_snowpacks), kinds;
    if (b->layer_kind) kinds.assign(b->layer_kind, b->layer_kind + (size_t)b->n_snowpacks * L);
    SarBatch d{};
    LrmBatch& lb = d.lrm;
    FoBatch& fo = lb.fo;
    fo.S = b->n_snowpacks; fo.Lmax = L; fo.F = 1; fo.n_theta = 1;
    fo.emmodel = b->emmodel; fo.micro = b->microstructure; fo.n_pairs = NP;
    fo.n_layers = nl.data();
    fo.thickness = b->thickness; fo.frac_volume = b->frac_volume; fo.temperature = b->temperature;
    fo.p1 = b->micro_p1; fo.p2 = b->micro_p2; fo.frequency = b->frequency; fo.liquid_water = b->liquid_water;
    fo.layer_kind = b->layer_kind ? kinds.data() : nullptr;
    fo.host_layer = b->host_layer; fo.host_coeff = b->host_iba_coeff;
    lb.ngate = p->ngate; lb.os = p->oversampling_time; lb.n_mu = 1;
    lb.oversampled = p->return_oversampled ? 1 : 0;
    lb.N = p->ngate * p->oversampling_time;
    lb.rows = 1; lb.out_rows = 1; lb.n_out = lb.oversampled ? lb.N : lb.ngate; lb.sar = 1;
    lb.altitude = p->altitude; lb.bandwidth = p->pulse_bandwidth; lb.nominal_gate = p->nominal_gate;
    lb.itf = p->boundary_values;
    d.ndoppler = p->ndoppler; d.osd = p->oversampling_doppler; d.ND = p->ndoppler * p->oversampling_doppler;
    d.out_rows = p->n_rows; d.n_tab = p->n_tables; d.n_t = lb.n_out; d.n_d = lb.oversampled ? d.ND : d.ndoppler;
    d.prf = p->pulse_repetition_frequency; d.wavelength = p->wavelength; d.velocity = p->velocity; d.alpha = p->alpha;
    d.pitch = p->pitch_angle; d.roll = p->roll_angle; d.sigma_p = p->sigma_p; d.theta_lim = p->theta_lim;
    d.gamma_x = p->gamma_x; d.gamma_y = p->gamma_y; d.l_gamma = p->l_gamma; d.lz = p->lz; d.pu = p->pu; d.nu_coherent = p->nu_coherent;
    if (h14) sar_h14_setup(d, p->slant_range_correction ? 1 : 0, p->delay_window_widening, p->h14_pu, p->h14_gamma, p->burst_duration);
    std::vector<int> tab_index(p->table_index, p->table_index + b->n_snowpacks);
    std::vector<int> row_map(p->row_map, p->row_map + (size_t)b->n_snowpacks * (2 * (L + 1) + 2));
    d.tab_sigma = p->table_sigma; d.tab_index = tab_index.data(); d.row_map = row_map.data();
    std::vector<double> stage((size_t)FO_ROWS * L * NP, 0.0), bs((size_t)L * NP, 0.0), prefix((size_t)NP * LRM_PREFIX_ROWS * (L + 1), 0.0);
    std::vector<double> tables((size_t)d.n_tab * (h14 ? 1 : 2) * lb.N * d.ND);
    std::vector<double> doppler(h14 ? (size_t)d.ND * d.N_wide : 0), kernel(h14 ? (size_t)d.n_tab * d.M : 0);
    // (each stage has exactly the LDS the launch gives it: a read past it is a read past the vector)
    std::vector<unsigned char> lds_vertical(lrm_vertical_lds_bytes(lb.N, L));
    std::vector<unsigned char> lds_combine(h14 ? sar_h14_combine_lds_bytes(lb.N, d.osd) : sar_combine_lds_bytes(lb.N, d.osd));
    fo.stage = stage.data(); fo.layer_out = layer_out;
    lb.bs = bs.data(); lb.prefix = prefix.data(); lb.vsd = vertical; lb.z_gate = z_gate; lb.status = status;
    d.tables = tables.data(); d.echo = echo; d.out = out;
    d.h14_doppler = doppler.data(); d.h14_kernel = kernel.data();
    LrmLane ln;
    ln.tid = 0; ln.nt = 1; ln.wsum = nullptr;
    for (long long i = 0; i < NP; ++i)
        for (int l = 0; l < L; ++l) lrm_layer_item(lb, i, l);
    for (long long i = 0; i < NP; ++i) { lrm_vertical_pair(lb, i, ln, lds_vertical.data()); sar_boundary_pair(d, i, 0, 1); }
    if (h14) {
        std::vector<unsigned char> l1(sar_h14_doppler_lds_bytes(d.ND)), l2(sar_h14_kernel_lds_bytes(d.M)), l3(sar_h14_delay_lds_bytes(d.N_wide, d.M));
        for (int n = 0; n < d.N_wide; ++n) sar_h14_doppler_row(d, n, 0, 1, l1.data());
        for (int t = 0; t < d.n_tab; ++t) sar_h14_kernel_table(d, t, 0, 1, l2.data());
        for (int t = 0; t < d.n_tab; ++t)
            for (int c = 0; c < d.ND; ++c) sar_h14_delay_column(d, t, c, 0, 1, l3.data());
        for (int n = 0; table && n < lb.N; ++n)
            for (int c = 0; c < d.ND; ++c) table[(size_t)n * d.ND + c] = tables[(size_t)c * lb.N + n];
    } else {
        for (long long k = 0; k < (long long)d.n_tab * lb.N * d.ND; ++k) sar_table_item(d, k);
    }
    for (long long i = 0; i < NP; ++i)
        for (int bin = 0; bin < d.ndoppler; ++bin) {
            if (h14) sar_combine_model<kSarHalimi14>(d, i, bin, 0, 1, lds_combine.data());
            else sar_combine_model<kSarDinardo18>(d, i, bin, 0, 1, lds_combine.data());
        }
    return 0;
}

extern "C" __attribute__((visibility("default")))
int32_t smrt_sar_host_run(const smrt_batch* b, const smrt_sar_params* p, double* out, int32_t* status, double* z_gate,
                          double* layer_out, double* vertical, double* echo) {
    return smrt_sar_host_run_table(b, p, out, status, z_gate, layer_out, vertical, echo, nullptr);
}

// what the C ABI answers to a batch before any device work: the message, or null
extern "C" __attribute__((visibility("default"))) const char* smrt_sar_host_refusal(const smrt_batch* b, const smrt_sar_params* p) {
    return solver_refusals::nadir_sar_altimetry(b, p);
}
