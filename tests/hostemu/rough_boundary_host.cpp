// The rough-boundary builder of the device (smrt_amd/csrc/rough_boundary_kernel.hpp) compiled for the CPU: its four block
// functions run under the fiber emulator, workgroup after workgroup, on every pair of the batch.  Built by build() and by
// tests/test_rough_device_cpu.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o librough_boundary_host.so rough_boundary_host.cpp
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../smrt_amd/csrc/rough_boundary_kernel.hpp"
#include "../../smrt_amd/csrc/dort_host_common.hpp"

using namespace smrt;

// what smrt_dort_upload answers to this batch: null, or the refusal
extern "C" __attribute__((visibility("default")))
const char* smrt_rough_host_refusal(const smrt_batch* b) { return smrt_host::validate(b); }

// Same outputs as smrt_dort_rough_matrices for the pairs of one upload, chosen as smrt_dort_upload / smrt_dort_upload_pairs
// choose them: the range [pair_begin, pair_begin + pair_count) of the global pairs f * S + s (pair_count < 0: to the end), or
// the pair_count pairs listed in `pairs` (pair_begin ignored).  The workspace is sized for the pairs of the upload and indexed
// by the position inside it; the outputs are sized for the whole batch and indexed by the global pair, as rough_prepare lays
// them out.  The caller hands zeroed arrays (slot filled with -1) sized for `slots` slots: pairs outside the upload stay so.
// order: the emulator's fiber order (0 forward, 1 reverse, 2 strided).  Returns the number of slots, or -1.
extern "C" __attribute__((visibility("default")))
int32_t smrt_rough_host_build_pairs(const smrt_batch* b, int32_t order, long long pair_begin, long long pair_count, const long long* pairs,
                                    int32_t* slot, double* itf, double* itf_coh, double* sub, double* sub_coh) {
    if (smrt_host::validate(b) || !b->rough_kind) return -1;
    const int S = b->n_snowpacks, L = b->n_layers_max, W = L + 1, nmax = b->n_max_stream;
    const long long all = (long long)S * b->n_frequencies;
    if (pairs) {
        pair_begin = 0;
        if (pair_count <= 0) return -1;
        for (long long i = 0; i < pair_count; ++i)
            if (pairs[i] < 0 || pairs[i] >= all) return -1;
    } else {
        if (pair_count < 0) pair_count = all - pair_begin;
        if (pair_begin < 0 || pair_count <= 0 || pair_begin + pair_count > all) return -1;
    }
    const long long np = pair_count;
    int slots = 0;
    for (int s = 0; s < S; ++s) {
        int c = 0;
        for (int l = 0; l < b->n_layers[s]; ++l) c += b->rough_kind[(size_t)s * W + l] != SMRT_ROUGH_NONE;
        slots = c > slots ? c : slots;
    }
    const int has_sub = smrt_host::rough_substrate(b) ? 1 : 0;
    if ((slots > 0 && (!slot || !itf || !itf_coh)) || (has_sub && (!sub || !sub_coh))) return -1;
    std::vector<double> gl(nmax), x(kRoughQuad / 2), wq(kRoughQuad / 2), quad(2 * kRoughQuad);
    smrt_host::gauss_legendre_positive(nmax, gl.data(), nullptr);
    smrt_host::gauss_legendre_positive(kRoughQuad / 2, x.data(), wq.data());
    for (int a = 0; a < kRoughQuad / 2; ++a) {
        quad[a] = 0.5 * (1.0 + x[a]); quad[kRoughQuad / 2 + a] = 0.5 * (1.0 - x[a]);
        quad[kRoughQuad + a] = quad[kRoughQuad + kRoughQuad / 2 + a] = 0.5 * wq[a];
    }
    std::vector<double> mu((size_t)np * W * nmax), w((size_t)np * W * nmax), eps((size_t)np * L * 2);
    std::vector<int> n((size_t)np * W, 0);
    std::vector<int> nl(b->n_layers, b->n_layers + S), kinds, rk(b->rough_kind, b->rough_kind + (size_t)S * W);
    if (b->layer_kind) kinds.assign(b->layer_kind, b->layer_kind + (size_t)S * L);
    RoughBatch r{};
    r.S = S; r.Lmax = L; r.F = b->n_frequencies; r.nmax = nmax; r.active = b->mode == SMRT_MODE_ACTIVE ? 1 : 0;
    r.nmodes = r.active ? b->m_max + 1 : 1;
    r.emmodel = b->emmodel; r.micro = b->microstructure;
    r.pair_begin = pair_begin; r.pair_count = np; r.pair_map = pairs;
    r.n_layers = nl.data(); r.frac_volume = b->frac_volume; r.temperature = b->temperature; r.p1 = b->micro_p1;
    r.p2 = b->micro_p2 ? b->micro_p2 : b->micro_p1; r.frequency = b->frequency;
    r.layer_kind = b->layer_kind ? kinds.data() : nullptr; r.liquid_water = b->liquid_water; r.host_layer = b->host_layer;
    r.gl_mu = gl.data(); r.quad = quad.data(); r.rough_kind = rk.data(); r.rough_params = b->rough_params;
    r.sub_p1 = b->substrate_p1; r.sub_p2 = b->substrate_p2; r.slots = slots; r.has_sub = has_sub;
    r.ws_mu = mu.data(); r.ws_w = w.data(); r.ws_n = n.data(); r.ws_eps = eps.data();
    r.itf_slot = slot; r.itf = itf; r.itf_coh = itf_coh; r.sub = sub; r.sub_coh = sub_coh;
    std::vector<double> lds(kRoughGoLds > kRoughHemiLds ? kRoughGoLds : kRoughHemiLds);
    int flags[2];
    for (long long ip = 0; ip < np; ++ip) emu::run_block(kRoughNT, order, [&]() { rough_setup_block(r, ip, flags); });
    const long long tasks = np * (slots + has_sub), tiles = ((long long)nmax * nmax + kRoughNT - 1) / kRoughNT;
    for (long long blk = 0; blk < tasks * 4 * tiles; ++blk)
        emu::run_block(kRoughNT, order, [&]() {
            switch (r.nmodes) {
                case 1: rough_go_block<1>(r, blk, lds.data()); break;
                case 2: rough_go_block<2>(r, blk, lds.data()); break;
                case 3: rough_go_block<3>(r, blk, lds.data()); break;
                case 4: rough_go_block<4>(r, blk, lds.data()); break;
                default: rough_go_block<5>(r, blk, lds.data()); break;
            }
        });
    for (long long blk = 0; blk < (tasks * 4 * nmax + kRoughNT - 1) / kRoughNT; ++blk)
        emu::run_block(kRoughNT, order, [&]() { rough_diag_block(r, blk); });
    for (long long blk = 0; blk < tasks * 2 * nmax; ++blk)
        emu::run_block(kRoughNT, order, [&]() { rough_hemi_block(r, blk, lds.data()); });
    return slots;
}

// every pair of the batch
extern "C" __attribute__((visibility("default")))
int32_t smrt_rough_host_build(const smrt_batch* b, int32_t order, int32_t* slot, double* itf, double* itf_coh, double* sub, double* sub_coh) {
    return smrt_rough_host_build_pairs(b, order, 0, -1, nullptr, slot, itf, itf_coh, sub, sub_coh);
}
