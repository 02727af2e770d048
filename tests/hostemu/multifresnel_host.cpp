// The device arithmetic of the multi-Fresnel thermal emission solver (smrt_amd/csrc/multifresnel_kernel.hpp) compiled for the
// CPU: its two per-item functions in plain loops.  Built by tests/host_build.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_multifresnel_host.so multifresnel_host.cpp
#include <cstdint>
#include <vector>

#include "host_batch.hpp"

using namespace smrt;

// Same batch, arguments and outputs as smrt_multifresnel_run_pairs over every pair, without a context.  Returns 0, or -1.
extern "C" __attribute__((visibility("default")))
int32_t smrt_multifresnel_host_run(const smrt_batch* b, const double* mu, double prune, int32_t prune_none, double* out,
                                   int32_t* status, int32_t* layers_used, double* tau_snowpack, double* layer_out) {
    if (!b || !mu || !out || !status || !layers_used || !tau_snowpack || !layer_out) return -1;
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE && b->substrate_kind != SMRT_SUBSTRATE_FLAT) return -1;
    const long long N = (long long)b->n_snowpacks * b->n_frequencies;
    host_batch::Inputs in;
    MfBatch d = solver_describe::multifresnel(b, mu, prune, prune_none, N);
    in.bind(b, nullptr, d);
    std::vector<double> stage(solver_describe::extents(d).stage, 0.0);
    d.mu = mu; d.sub_T = b->substrate_temperature;
    d.stage = stage.data(); d.out = out; d.status = status; d.layers_used = layers_used; d.tau_snowpack = tau_snowpack;
    d.layer_out = layer_out;
    for (long long i = 0; i < N; ++i)
        for (int l = 0; l <= d.Lmax; ++l) multifresnel_layer_item(d, i, l);
    for (long long i = 0; i < N; ++i)
        for (int t = 0; t < d.n_theta; ++t) multifresnel_chain_item(d, i, t);
    return 0;
}
