// The device arithmetic of the nadir LRM altimetry solver (smrt_amd/csrc/nadir_lrm_altimetry_kernel.hpp) compiled for the CPU:
// a "workgroup" of one thread, scans as running sums.  Built by tests/host_build.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_lrm_host.so nadir_lrm_altimetry_host.cpp
#include <cstdint>
#include <vector>

#include "host_batch.hpp"

using namespace smrt;

namespace {
// What both entry points set up: the inputs, the buffers of the layer kernel, and its loop.
struct LrmHost {
    host_batch::Inputs in;
    LrmBatch d;
    solver_describe::LrmExtents n;
    std::vector<double> stage, bs;
    LrmHost(const smrt_batch* b, const LrmBatch& described, double* layer_out)
        : d(described), n(solver_describe::extents(d)), stage(n.stage, 0.0), bs(n.bs, 0.0) {
        in.bind(b, nullptr, d.fo);
        d.fo.stage = stage.data(); d.fo.layer_out = layer_out; d.bs = bs.data();
    }
    void layers() const {
        for (long long i = 0; i < d.fo.n_pairs; ++i)
            for (int l = 0; l < d.fo.Lmax; ++l) lrm_layer_item(d, i, l);
    }
};
}  // namespace

// Same batch, parameters and outputs as smrt_lrm_run_pairs over every pair, without a context.  Returns 0, or -1.
extern "C" __attribute__((visibility("default")))
int32_t smrt_lrm_host_run(const smrt_batch* b, const smrt_lrm_params* p, double* out, int32_t* status, double* z_gate,
                          double* layer_out, double* vertical) {
    if (!b || !p || !out || !status || !z_gate || !layer_out || !vertical) return -1;
    if (p->n_mu < 1 || (p->n_mu > 1 && (p->skip_pfs_convolution || p->sigma_surface))) return -1;
    LrmHost h(b, solver_describe::nadir_lrm_altimetry(b, p, (long long)b->n_snowpacks * b->n_frequencies), layer_out);
    LrmBatch& d = h.d;
    d.t_inc = p->t_inc; d.sigma_surface = p->sigma_surface; d.surface_slope = p->surface_slope; d.itf = p->interface_values;
    std::vector<double> prefix(h.n.prefix, 0.0);
    std::vector<unsigned char> lds(h.n.lds_vertical + h.n.lds_waveform);
    d.prefix = prefix.data(); d.vsd = vertical; d.out = out; d.z_gate = z_gate; d.status = status;
    LrmLane ln{0, 1, nullptr};
    h.layers();
    for (long long i = 0; i < d.fo.n_pairs; ++i) lrm_vertical_pair(d, i, ln, lds.data());
    for (long long i = 0; i < d.fo.n_pairs; ++i)
        for (int r = 0; r < d.out_rows; ++r) lrm_waveform_item(d, i, r, ln, lds.data());
    return 0;
}

// The layer scalars alone (smrt_lrm_layers): layer_out [pairs][n_layers_max][5]
extern "C" __attribute__((visibility("default")))
int32_t smrt_lrm_host_layers(const smrt_batch* b, double* layer_out) {
    if (!b || !layer_out) return -1;
    LrmBatch d{};
    d.fo = solver_describe::altimetry_layers(b, b->n_frequencies, (long long)b->n_snowpacks * b->n_frequencies);
    LrmHost(b, d, layer_out).layers();
    return 0;
}

// I0 as the kernels compute it (held to scipy.special.i0 by the tests)
extern "C" __attribute__((visibility("default"))) double smrt_lrm_host_i0(double x) { return lrm_i0(x); }
