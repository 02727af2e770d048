// The device arithmetic of the nadir LRM altimetry solver (smrt_amd/csrc/nadir_lrm_altimetry_kernel.hpp) compiled for the CPU:
// a "workgroup" of one thread, scans as running sums.  Built by tests/test_nadir_lrm_altimetry_cpu.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_lrm_host.so nadir_lrm_altimetry_host.cpp
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../smrt_amd/csrc/nadir_lrm_altimetry_kernel.hpp"
#include "../../include/smrt_dort.h"

using namespace smrt;

// Same batch, parameters and outputs as smrt_lrm_run_pairs over every pair, without a context.  Returns 0, or -1.
extern "C" __attribute__((visibility("default")))
int32_t smrt_lrm_host_run(const smrt_batch* b, const smrt_lrm_params* p, double* out, int32_t* status, double* z_gate,
                          double* layer_out, double* vertical) {
    if (!b || !p || !out || !status || !z_gate || !layer_out || !vertical) return -1;
    if (p->n_mu < 1 || (p->n_mu > 1 && (p->skip_pfs_convolution || p->sigma_surface))) return -1;
    const long long NP = (long long)b->n_snowpacks * b->n_frequencies;
    const int L = b->n_layers_max;
    std::vector<int> nl(b->n_layers, b->n_layers + b->n_snowpacks), kinds;
    if (b->layer_kind) kinds.assign(b->layer_kind, b->layer_kind + (size_t)b->n_snowpacks * L);
    LrmBatch d{};
    FoBatch& fo = d.fo;
    fo.S = b->n_snowpacks; fo.Lmax = L; fo.F = b->n_frequencies; fo.n_theta = 1;
    fo.emmodel = b->emmodel; fo.micro = b->microstructure; fo.n_pairs = NP;
    fo.n_layers = nl.data();
    fo.thickness = b->thickness; fo.frac_volume = b->frac_volume; fo.temperature = b->temperature;
    fo.p1 = b->micro_p1; fo.p2 = b->micro_p2; fo.frequency = b->frequency; fo.liquid_water = b->liquid_water;
    fo.layer_kind = b->layer_kind ? kinds.data() : nullptr;
    fo.host_layer = b->host_layer; fo.host_coeff = b->host_iba_coeff;
    d.ngate = p->ngate; d.os = p->oversampling; d.n_mu = p->n_mu; d.shift = p->shift;
    d.contributions = p->return_contributions ? 1 : 0; d.oversampled = p->return_oversampled ? 1 : 0;
    d.skip_pfs = p->skip_pfs_convolution ? 1 : 0;
    d.N = p->ngate * p->oversampling;
    d.rows = p->n_mu > 1 ? 2 * p->n_mu + 1 : p->return_contributions ? 3 : 1;
    d.out_rows = p->return_contributions ? 3 : p->skip_pfs_convolution ? d.rows : 1;
    d.n_out = d.oversampled ? d.N : d.ngate;
    d.altitude = p->altitude; d.bandwidth = p->pulse_bandwidth; d.gain = p->antenna_gain; d.gamma = p->gamma;
    d.off_nadir = p->off_nadir_angle; d.nominal_gate = p->nominal_gate; d.pulse_sigma = p->pulse_sigma;
    d.t_inc = p->t_inc; d.sigma_surface = p->sigma_surface; d.surface_slope = p->surface_slope; d.itf = p->interface_values;
    std::vector<double> stage((size_t)FO_ROWS * L * NP, 0.0), bs((size_t)L * NP, 0.0), prefix((size_t)NP * LRM_PREFIX_ROWS * (L + 1), 0.0);
    std::vector<unsigned char> lds(lrm_vertical_lds_bytes(d.N, L) + lrm_waveform_lds_bytes(d.N, d.n_mu));
    fo.stage = stage.data(); fo.layer_out = layer_out;
    d.bs = bs.data(); d.prefix = prefix.data(); d.vsd = vertical; d.out = out; d.z_gate = z_gate; d.status = status;
    LrmLane ln;
    ln.tid = 0; ln.nt = 1; ln.wsum = nullptr;
    for (long long i = 0; i < NP; ++i)
        for (int l = 0; l < L; ++l) lrm_layer_item(d, i, l);
    for (long long i = 0; i < NP; ++i) lrm_vertical_pair(d, i, ln, lds.data());
    for (long long i = 0; i < NP; ++i)
        for (int r = 0; r < d.out_rows; ++r) lrm_waveform_item(d, i, r, ln, lds.data());
    return 0;
}

// The layer scalars alone (smrt_lrm_layers): layer_out [pairs][n_layers_max][5]
extern "C" __attribute__((visibility("default")))
int32_t smrt_lrm_host_layers(const smrt_batch* b, double* layer_out) {
    if (!b || !layer_out) return -1;
    const long long NP = (long long)b->n_snowpacks * b->n_frequencies;
    const int L = b->n_layers_max;
    std::vector<int> nl(b->n_layers, b->n_layers + b->n_snowpacks), kinds;
    if (b->layer_kind) kinds.assign(b->layer_kind, b->layer_kind + (size_t)b->n_snowpacks * L);
    LrmBatch d{};
    FoBatch& fo = d.fo;
    fo.S = b->n_snowpacks; fo.Lmax = L; fo.F = b->n_frequencies; fo.n_theta = 1;
    fo.emmodel = b->emmodel; fo.micro = b->microstructure; fo.n_pairs = NP;
    fo.n_layers = nl.data();
    fo.thickness = b->thickness; fo.frac_volume = b->frac_volume; fo.temperature = b->temperature;
    fo.p1 = b->micro_p1; fo.p2 = b->micro_p2; fo.frequency = b->frequency; fo.liquid_water = b->liquid_water;
    fo.layer_kind = b->layer_kind ? kinds.data() : nullptr;
    fo.host_layer = b->host_layer; fo.host_coeff = b->host_iba_coeff;
    std::vector<double> stage((size_t)FO_ROWS * L * NP, 0.0), bs((size_t)L * NP, 0.0);
    fo.stage = stage.data(); fo.layer_out = layer_out; d.bs = bs.data();
    for (long long i = 0; i < NP; ++i)
        for (int l = 0; l < L; ++l) lrm_layer_item(d, i, l);
    return 0;
}

// I0 as the kernels compute it (held to scipy.special.i0 by the tests)
extern "C" __attribute__((visibility("default"))) double smrt_lrm_host_i0(double x) { return lrm_i0(x); }
