// The device arithmetic of the iterative second-order solver (smrt_amd/csrc/second_order_kernel.hpp, on top of
// first_order_kernel.hpp) compiled for the CPU: the per-item functions in plain loops, the wavefront function of the
// integrals under the fiber emulator (64 fibers).  Built by tests/host_build.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_second_order_host.so second_order_host.cpp
#include <cstdint>
#include <vector>

#include "host_batch.hpp"

using namespace smrt;

template <int M>
static void run_units(const So2Batch& d, int order) {
    const int L = d.fo.Lmax, T = d.fo.n_theta;
    for (long long r = 0; r < d.chunk_count; ++r)
        for (int n = 0; n < L; ++n)
            for (int t = 0; t < T; ++t) {
                emu::run_block(SMRT_LANES, order, [&] { second_order_integral_unit<M>(d, r, n, -1, t, tid()); });
                for (int m = 0; d.interlayer && m < L; ++m)
                    emu::run_block(SMRT_LANES, order, [&] { second_order_integral_unit<M>(d, r, n, m, t, tid()); });
            }
}

// Same arguments and outputs as smrt_second_order_run_pairs over every pair, without a context and in one chunk.  `order`:
// the visiting order of the fibers (0 forward, 1 reverse, 2 strided).  Returns 0, or -1.
extern "C" __attribute__((visibility("default")))
int32_t smrt_second_order_host_run(const smrt_batch* b, const smrt_second_order_extras* x, int32_t order, double* out, int32_t* status,
                                   double* layer_out, double* backscatter_layer, double* diag) {
    if (!b || !out || !status || !backscatter_layer) return -1;
    if (b->n_max_stream < 2 || b->m_max < 1 || b->m_max > kSo2MaxModes) return -1;
    const long long N = (long long)b->n_snowpacks * b->n_frequencies;
    const smrt_first_order_extras* x1 = x ? x->first_order : nullptr;
    host_batch::Inputs in;
    So2Batch d = solver_describe::second_order(b, x, N);
    FoBatch& f = d.fo;
    in.bind(b, nullptr, f);
    const int L = f.Lmax, T = f.n_theta;
    const solver_describe::FoExtents nf = solver_describe::extents(f);
    const solver_describe::So2Extents n = solver_describe::extents(d, (size_t)N);   // one chunk
    std::vector<double> stage(nf.stage, 0.0), fo_out(nf.out), fo_lb(nf.layer_backscatter), carry(nf.carry, 0.0), gl(n.gl_mu);
    f.theta = b->theta;
    if (x1 && x1->host_interface_slot) { f.itf_slot = x1->host_interface_slot; f.itf_values = x1->host_interface_values; }
    f.stage = stage.data(); f.out = fo_out.data(); f.status = status;
    f.layer_out = layer_out; f.layer_backscatter = fo_lb.data(); f.diag = diag; f.carry = carry.data();
    for (long long i = 0; i < N; ++i)
        for (int l = 0; l < L; ++l) first_order_layer_item(f, i, l);
    for (long long i = 0; i < N; ++i)
        for (int t = 0; t < T; ++t) first_order_angle_item(f, i, t);
    smrt_host::gauss_legendre_positive(d.nmax, gl.data(), nullptr);
    d.chunk_begin = 0; d.chunk_count = N;
    d.gl_mu = gl.data(); d.sub_modes = x ? x->substrate_diffuse_modes : nullptr;
    std::vector<int> nstream(n.nstream, 0);
    std::vector<double> streams(n.streams, 0.0), integ(n.integ, 0.0);
    d.nstream = nstream.data(); d.streams = streams.data(); d.integ = integ.data();
    d.out = out; d.layer_backscatter = backscatter_layer;
    for (long long i = 0; i < N; ++i)
        for (int l = 0; l < L; ++l) second_order_stream_item(d, i, l);
    if (d.m_max <= 2) run_units<2>(d, order);
    else if (d.m_max <= 3) run_units<3>(d, order);
    else if (d.m_max <= 5) run_units<5>(d, order);
    else run_units<8>(d, order);
    for (long long i = 0; i < N; ++i)
        for (int t = 0; t < T; ++t) second_order_walk_item(d, i, t);
    return 0;
}

// The device's closed-form factors, one by one (`which`: 'A' .. 'F'), for the test of their values at and next to coincident
// cosines.  A, B read (ke_n, tau_n); E, F read (ke_n, tau_n) and tau_r as the optical depth down to the ground.
extern "C" __attribute__((visibility("default")))
double smrt_second_order_host_coef(int32_t which, double mi, double mu, double ke_n, double ke_m, double tau_n, double tau_m,
                                   double tau_r) {
    switch (which) {
        case 'A': return so2_coef_A(mi, mu, ke_n, tau_n);
        case 'B': return so2_coef_B(mi, mu, ke_n, tau_n);
        case 'C': return so2_coef_C(mi, mu, ke_n, ke_m, tau_n, tau_m, tau_r);
        case 'D': return so2_coef_D(mi, mu, ke_n, ke_m, tau_n, tau_m, tau_r);
        case 'E': return so2_coef_E(mi, mu, ke_n, tau_n, tau_r);
        case 'F': return so2_coef_F(mi, mu, ke_n, tau_n, tau_r);
    }
    return NAN;
}
