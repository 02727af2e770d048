// The device arithmetic of the successive-order backscatter solver (smrt_amd/csrc/successive_order_active_kernel.hpp) compiled
// for the CPU: the per-(pair, layer) and per-output-element functions in plain loops, the two workgroup functions under the
// fiber emulator (256 fibers, the MFMA in its gfx950 lane layout).  Built by tests/host_build.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_so_active_host.so successive_order_active_host.cpp
#include <cstdint>
#include <vector>

#include "host_batch.hpp"

using namespace smrt;

// Same batch, options and outputs as smrt_so_active_run_pairs over every pair, without a context and without
// a budget: one chunk.  `order`: the visiting order of the fibers (0 forward, 1 reverse, 2 strided).  Returns 0, or -1.
extern "C" __attribute__((visibility("default")))
int32_t smrt_so_active_host_run(const smrt_batch* b, int32_t n_iter, double rtol, int32_t n_theta_inc,
                                              const double* theta_inc, int32_t npi, int32_t m_max, int32_t order, double* out,
                                              int32_t* status, double* layer_out, double* streams, int32_t* sublayers,
                                              double* max_radiance, int32_t* orders) {
    if (!b || !out || !status || !layer_out || !streams || !sublayers || !max_radiance || !orders || n_iter < 1) return -1;
    if (b->n_max_stream < 2 || b->n_max_stream > kSoMaxStream || n_theta_inc < 1 || npi < 1 || npi > 3 || m_max < 0) return -1;
    const long long N = (long long)b->n_snowpacks * b->n_frequencies;
    host_batch::Inputs in;
    SoaBatch a = solver_describe::successive_order_active(b, n_iter, rtol, n_theta_inc, npi, m_max, N);
    SoBatch& d = a.so;
    in.bind(b, nullptr, d);
    const solver_describe::SoaExtents n = solver_describe::extents(a);
    const int L = d.Lmax, M = m_max + 1, NP = m_max + 2;
    std::vector<int> nsub(n.nsub), nstream(n.nstream, 0), inc(n.inc, 0);
    std::vector<double> stage(n.stage, 0.0), vec(n.vec, 0.0), air(n.air, 0.0), back(n.back, 0.0), gl(n.gl_mu);
    smrt_host::gauss_legendre_positive(d.nmax, gl.data(), nullptr);
    d.chunk_begin = 0; d.chunk_count = N;
    d.theta = theta_inc; d.gl_mu = gl.data();
    d.stage = stage.data(); d.nsub = nsub.data(); d.nstream = nstream.data(); d.vec = vec.data();
    d.out = out; d.status = status; d.layer_out = layer_out; d.streams = streams; d.maxrad = max_radiance; d.orders = orders;
    a.air = air.data(); a.back = back.data(); a.inc = inc.data();
    for (long long i = 0; i < N; ++i)
        for (int l = 0; l < L; ++l) so_layer_item(d, i, l);
    std::vector<long long> ws_off(n.ws_off);
    long long total = 0;
    for (long long i = 0; i < N; ++i) {
        long long n_sub = 0, n_lay = 0;
        for (int l = 0; l < L; ++l) { n_sub += nsub[(size_t)i * L + l]; n_lay += nsub[(size_t)i * L + l] > 0; sublayers[i * L + l] = nsub[(size_t)i * L + l]; }
        ws_off[(size_t)i] = total;
        total += NP * soa_pass_doubles(n_sub, n_lay, a.Cmax, d.nmax);
    }
    std::vector<double> wt((size_t)N * n.wt_pair, 0.0), ws((size_t)total, 0.0), lds(n.lds_sweep / sizeof(double), 0.0);
    d.wt = wt.data(); d.ws = ws.data(); d.ws_off = ws_off.data();
    for (long long i = 0; i < N; ++i)
        for (int m = 0; m < M; ++m)
            for (int l = 0; l < L; ++l) emu::run_block(kSoaThreads, order, [&] { soa_prep_item<kSoaThreads>(a, i, l, m); });
    for (long long i = 0; i < N; ++i)
        for (int pass = 0; pass < NP; ++pass) emu::run_block(kSoaThreads, order, [&] { soa_sweep_pass<kSoaThreads>(a, i, pass, lds.data()); });
    const int row = 9 * n_theta_inc * (n_iter + 1);
    for (long long i = 0; i < N; ++i)
        for (int e = 0; e < row; ++e) soa_combine_item(a, i, e);
    return 0;
}

// The incident streams of soa_incident_streams on a caller's descending cosines; returns their number.
extern "C" __attribute__((visibility("default")))
int32_t smrt_so_active_host_incident(const double* outmu, int32_t n_air, const double* theta_inc, int32_t n_theta_inc,
                                                   int32_t* list) {
    return soa_incident_streams(outmu, n_air, theta_inc, n_theta_inc, list);
}
