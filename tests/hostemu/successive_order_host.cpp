// The device arithmetic of the successive-order solver (smrt_amd/csrc/successive_order_kernel.hpp) compiled for the CPU:
// the per-(pair, layer) function in a plain loop, the two workgroup functions under the fiber emulator (256 fibers, the
// MFMA in its gfx950 lane layout).  Built by tests/host_build.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_successive_order_host.so successive_order_host.cpp
#include <cstdint>
#include <vector>

#include "host_batch.hpp"

using namespace smrt;

// Same batch, options and outputs as smrt_successive_order_run_pairs over every pair, without a context and without a
// budget: one chunk.  `order`: the visiting order of the fibers (0 forward, 1 reverse, 2 strided).  Returns 0, or -1.
extern "C" __attribute__((visibility("default")))
int32_t smrt_successive_order_host_run(const smrt_batch* b, int32_t n_iter, double rtol, int32_t order, double* out, int32_t* status,
                                       double* layer_out, double* streams, int32_t* sublayers, double* max_radiance, int32_t* orders) {
    if (!b || !out || !status || !layer_out || !streams || !sublayers || !max_radiance || !orders || n_iter < 1) return -1;
    if (b->n_max_stream < 2 || b->n_max_stream > kSoMaxStream) return -1;
    const long long N = (long long)b->n_snowpacks * b->n_frequencies;
    host_batch::Inputs in;
    SoBatch d = solver_describe::successive_order(b, n_iter, rtol, N);
    in.bind(b, nullptr, d);
    const solver_describe::SoExtents n = solver_describe::extents(d);
    const int L = d.Lmax, Dh = 2 * d.nmax, Dp = so_dp(d.nmax);
    std::vector<int> nsub(n.nsub), nstream(n.nstream, 0);
    std::vector<double> stage(n.stage, 0.0), vec(n.vec, 0.0), srcterm(n.srcterm, 0.0), gl(n.gl_mu);
    std::vector<double> subT(b->n_snowpacks, 0.0);   // (zeros where the caller gives no substrate temperature)
    for (int s = 0; s < b->n_snowpacks && b->substrate_temperature; ++s) subT[s] = b->substrate_temperature[s];
    smrt_host::gauss_legendre_positive(d.nmax, gl.data(), nullptr);
    d.chunk_begin = 0; d.chunk_count = N;
    d.theta = b->theta; d.sub_T = subT.data(); d.gl_mu = gl.data();
    d.stage = stage.data(); d.nsub = nsub.data(); d.nstream = nstream.data(); d.vec = vec.data(); d.srcterm = srcterm.data();
    d.out = out; d.status = status; d.layer_out = layer_out; d.streams = streams; d.maxrad = max_radiance; d.orders = orders;
    for (long long i = 0; i < N; ++i)
        for (int l = 0; l < L; ++l) so_layer_item(d, i, l);
    std::vector<long long> ws_off(n.ws_off);
    long long total = 0;
    for (long long i = 0; i < N; ++i) {
        long long n_sub = 0, n_lay = 0;
        for (int l = 0; l < L; ++l) { n_sub += nsub[(size_t)i * L + l]; n_lay += nsub[(size_t)i * L + l] > 0; sublayers[i * L + l] = nsub[(size_t)i * L + l]; }
        ws_off[(size_t)i] = total;
        total += (2 * n_sub + n_lay) * Dp + 2 * n_lay * Dh;
    }
    std::vector<double> wt((size_t)N * n.wt_pair, 0.0), ws((size_t)total, 0.0), lds(n.lds_sweep / sizeof(double), 0.0);
    d.wt = wt.data(); d.ws = ws.data(); d.ws_off = ws_off.data();
    for (long long i = 0; i < N; ++i)
        for (int l = 0; l < L; ++l) emu::run_block(kSoThreads, order, [&] { so_prep_item<kSoThreads>(d, i, l); });
    for (long long i = 0; i < N; ++i) emu::run_block(kSoThreads, order, [&] { so_sweep_pair<kSoThreads>(d, i, lds.data()); });
    return 0;
}
