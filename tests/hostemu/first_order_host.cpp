// The device arithmetic of the iterative first-order solver (smrt_amd/csrc/first_order_kernel.hpp) compiled for the CPU:
// the two per-item functions in plain loops over the items their kernels give one lane each.  Built by
// tests/host_build.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_first_order_host.so first_order_host.cpp
#include <cstdint>
#include <vector>

#include "host_batch.hpp"

using namespace smrt;

// Same arguments and outputs as smrt_first_order_run_pairs, without a context.  Returns 0, or -1 on null arguments.
extern "C" __attribute__((visibility("default")))
int32_t smrt_first_order_host_run(const smrt_batch* b, const smrt_first_order_extras* x, const int64_t* pairs, int64_t n_pairs,
                                  double* out, int32_t* status, double* layer_out, double* backscatter_layer, double* diag) {
    if (!b || !out || !status) return -1;
    if (!pairs) n_pairs = (int64_t)b->n_snowpacks * b->n_frequencies;
    host_batch::Inputs in;
    FoBatch d = solver_describe::first_order(b, x, n_pairs);
    in.bind(b, pairs, d);
    std::vector<double> stage(solver_describe::extents(d).stage, 0.0);
    d.theta = b->theta;
    if (x && x->host_interface_slot) { d.itf_slot = x->host_interface_slot; d.itf_values = x->host_interface_values; }
    d.host_phase = x ? x->host_phase_samples : nullptr;
    d.stage = stage.data(); d.out = out; d.status = status;
    d.layer_out = layer_out; d.layer_backscatter = backscatter_layer; d.diag = diag;
    for (long long i = 0; i < n_pairs; ++i)
        for (int l = 0; l < d.Lmax; ++l) first_order_layer_item(d, i, l);
    for (long long i = 0; i < n_pairs; ++i)
        for (int t = 0; t < d.n_theta; ++t) first_order_angle_item(d, i, t);
    return 0;
}
