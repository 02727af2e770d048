// The device arithmetic of the multi-Fresnel thermal emission solver (smrt_amd/csrc/multifresnel_kernel.hpp) compiled for the
// CPU: its two per-item functions in plain loops.  Built by tests/test_multifresnel_cpu.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_multifresnel_host.so multifresnel_host.cpp
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../smrt_amd/csrc/multifresnel_kernel.hpp"
#include "../../include/smrt_dort.h"

using namespace smrt;

// Same batch, arguments and outputs as smrt_multifresnel_run_pairs over every pair, without a context.  Returns 0, or -1.
extern "C" __attribute__((visibility("default")))
int32_t smrt_multifresnel_host_run(const smrt_batch* b, const double* mu, double prune, int32_t prune_none, double* out,
                                   int32_t* status, int32_t* layers_used, double* tau_snowpack, double* layer_out) {
    if (!b || !mu || !out || !status || !layers_used || !tau_snowpack || !layer_out) return -1;
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE && b->substrate_kind != SMRT_SUBSTRATE_FLAT) return -1;
    const long long N = (long long)b->n_snowpacks * b->n_frequencies;
    const int L = b->n_layers_max;
    std::vector<int> nl(b->n_layers, b->n_layers + b->n_snowpacks), kinds;
    if (b->layer_kind) kinds.assign(b->layer_kind, b->layer_kind + (size_t)b->n_snowpacks * L);
    std::vector<double> stage((size_t)MF_ROWS * (L + 1) * N, 0.0);
    MfBatch d{};
    d.S = b->n_snowpacks; d.Lmax = L; d.F = b->n_frequencies; d.n_theta = b->n_theta;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.sub_kind = b->substrate_kind;
    d.prune = prune_none ? INFINITY : prune;
    d.steepest = 0;
    for (int t = 1; t < b->n_theta; ++t) if (mu[t] > mu[d.steepest]) d.steepest = t;
    d.n_pairs = N;
    d.n_layers = nl.data();
    d.thickness = b->thickness; d.frac_volume = b->frac_volume; d.temperature = b->temperature;
    d.p1 = b->micro_p1; d.p2 = b->micro_p2; d.frequency = b->frequency; d.mu = mu; d.liquid_water = b->liquid_water;
    d.layer_kind = b->layer_kind ? kinds.data() : nullptr;
    d.sub_p1 = b->substrate_p1; d.sub_p2 = b->substrate_p2; d.sub_T = b->substrate_temperature;
    d.stage = stage.data(); d.out = out; d.status = status; d.layers_used = layers_used; d.tau_snowpack = tau_snowpack;
    d.layer_out = layer_out;
    for (long long i = 0; i < N; ++i)
        for (int l = 0; l <= L; ++l) multifresnel_layer_item(d, i, l);
    for (long long i = 0; i < N; ++i)
        for (int t = 0; t < b->n_theta; ++t) multifresnel_chain_item(d, i, t);
    return 0;
}
