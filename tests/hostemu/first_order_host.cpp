// The device arithmetic of the iterative first-order solver (smrt_amd/csrc/first_order_kernel.hpp) compiled for the CPU:
// the two per-item functions in plain loops over the items their kernels give one lane each.  Built by
// tests/test_first_order_cpu.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_first_order_host.so first_order_host.cpp
#include <cstdint>
#include <vector>

#include "../../smrt_amd/csrc/first_order_kernel.hpp"
#include "../../include/smrt_dort.h"

using namespace smrt;

// Same arguments and outputs as smrt_first_order_run_pairs, without a context.  Returns 0, or -1 on null arguments.
extern "C" __attribute__((visibility("default")))
int32_t smrt_first_order_host_run(const smrt_batch* b, const smrt_first_order_extras* x, const int64_t* pairs, int64_t n_pairs,
                                  double* out, int32_t* status, double* layer_out, double* backscatter_layer, double* diag) {
    if (!b || !out || !status) return -1;
    if (!pairs) n_pairs = (int64_t)b->n_snowpacks * b->n_frequencies;
    std::vector<long long> map(pairs ? pairs : nullptr, pairs ? pairs + n_pairs : nullptr);
    std::vector<double> stage((size_t)FO_ROWS * b->n_layers_max * n_pairs, 0.0);
    std::vector<int> nl(b->n_layers, b->n_layers + b->n_snowpacks), kinds;
    if (b->layer_kind) kinds.assign(b->layer_kind, b->layer_kind + (size_t)b->n_snowpacks * b->n_layers_max);
    std::vector<int> slots;
    FoBatch d{};
    d.S = b->n_snowpacks; d.Lmax = b->n_layers_max; d.F = b->n_frequencies; d.n_theta = b->n_theta;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.sub_kind = b->substrate_kind;
    d.n_pairs = n_pairs;
    d.pair_map = pairs ? map.data() : nullptr;
    d.n_layers = nl.data();
    d.thickness = b->thickness; d.frac_volume = b->frac_volume; d.temperature = b->temperature;
    d.p1 = b->micro_p1; d.p2 = b->micro_p2; d.frequency = b->frequency; d.theta = b->theta; d.liquid_water = b->liquid_water;
    d.layer_kind = b->layer_kind ? kinds.data() : nullptr;
    d.host_layer = b->host_layer; d.host_coeff = b->host_iba_coeff;
    d.sub_p1 = b->substrate_p1; d.sub_p2 = b->substrate_p2;
    if (x && x->host_interface_slot) {
        const size_t n = (size_t)b->n_frequencies * b->n_snowpacks * (b->n_layers_max + 1);
        slots.assign(x->host_interface_slot, x->host_interface_slot + n);
        d.itf_slot = slots.data(); d.itf_values = x->host_interface_values; d.n_slots = x->n_interface_slots;
    }
    d.host_phase = x ? x->host_phase_samples : nullptr;
    d.stage = stage.data(); d.out = out; d.status = status;
    d.layer_out = layer_out; d.layer_backscatter = backscatter_layer; d.diag = diag;
    for (long long i = 0; i < n_pairs; ++i)
        for (int l = 0; l < d.Lmax; ++l) first_order_layer_item(d, i, l);
    for (long long i = 0; i < n_pairs; ++i)
        for (int t = 0; t < d.n_theta; ++t) first_order_angle_item(d, i, t);
    return 0;
}
