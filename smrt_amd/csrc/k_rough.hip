// Rough boundaries on the device (rough_boundary_kernel.hpp): the kernels, their buffers on the context and the builder that
// upload_impl (dort_hip.hip) calls for a batch with rough_kind -- it fills the arrays the dense composition reads
// (host_interface*, host_substrate*) for the pairs of the upload and points the DevBatch at them.
#include <climits>
#include <vector>

#include "dort_ctx.hpp"
#include "rough_boundary_kernel.hpp"
#include "solver_host.hpp"

using namespace smrt;

__global__ __launch_bounds__(kRoughNT) void rough_setup_kernel(RoughBatch b) {
    __shared__ int flags[2];
    rough_setup_block(b, (long long)blockIdx.x, flags);
}

template <int MM>
__global__ __launch_bounds__(kRoughNT) void rough_go_kernel(RoughBatch b) {
    __shared__ double lds[(2 + MM) * (kRoughHalf + 1)];
    rough_go_block<MM>(b, (long long)blockIdx.x, lds);
}

__global__ __launch_bounds__(kRoughNT) void rough_diag_kernel(RoughBatch b) { rough_diag_block(b, (long long)blockIdx.x); }

__global__ __launch_bounds__(kRoughNT) void rough_hemi_kernel(RoughBatch b) {
    __shared__ double lds[kRoughHemiLds];
    rough_hemi_block(b, (long long)blockIdx.x, lds);
}

struct RoughState : solver_host::SolverState {
    DevBuf &kind = buf(), &par = buf(), &mu = buf(), &w = buf(), &n = buf(), &eps = buf(), &quad = buf(), &sub1 = buf(), &sub2 = buf();
    bool quad_ready = false;
};

namespace smrt_launch {

void rough_release(smrt_dort_ctx* ctx) { solver_host::release(ctx->rough); }

int rough_prepare(smrt_dort_ctx* ctx, const smrt_batch* b, DevBatch& d) {
    if (!ctx->rough) ctx->rough = new RoughState();
    RoughState* st = ctx->rough;
    const int S = b->n_snowpacks, L = b->n_layers_max, W = L + 1, nmax = b->n_max_stream;
    const size_t FS = (size_t)S * b->n_frequencies, NE = 3 * (size_t)nmax;
    const int nmodes = ctx->active ? b->m_max + 1 : 1;
    int slots = 0;
    for (int s = 0; s < S; ++s) {
        int c = 0;
        for (int l = 0; l < b->n_layers[s]; ++l) c += b->rough_kind[(size_t)s * W + l] != SMRT_ROUGH_NONE;
        slots = c > slots ? c : slots;
    }
    const int has_sub = smrt_host::rough_substrate(b) ? 1 : 0;
    RoughBatch r{};
    r.S = S; r.Lmax = L; r.F = b->n_frequencies; r.nmax = nmax; r.nmodes = nmodes; r.active = ctx->active ? 1 : 0;
    r.emmodel = b->emmodel; r.micro = b->microstructure;
    r.pair_begin = d.pair_begin; r.pair_count = d.pair_count; r.pair_map = d.pair_map;
    r.n_layers = d.n_layers; r.frac_volume = d.frac_volume; r.temperature = d.temperature; r.p1 = d.p1; r.p2 = d.p2;
    r.frequency = d.frequency; r.layer_kind = d.layer_kind; r.liquid_water = d.liquid_water; r.host_layer = d.host_layer;
    r.gl_mu = d.gl_mu;
    r.slots = slots; r.has_sub = has_sub;
    HIPCHK(st->kind.reserve(sizeof(int32_t) * (size_t)S * W));
    HIPCHK(st->par.reserve(sizeof(double) * (size_t)S * W * 4));
    HIPCHK(hipMemcpyAsync(st->kind.p, b->rough_kind, sizeof(int32_t) * (size_t)S * W, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(st->par.p, b->rough_params, sizeof(double) * (size_t)S * W * 4, hipMemcpyHostToDevice, ctx->stream));
    r.rough_kind = (const int*)st->kind.p; r.rough_params = (const double*)st->par.p;
    if (!st->quad_ready) {   // the 128-point Gauss-Legendre rule on [0, 1], from the library's own routine, uploaded once
        std::vector<double> x(kRoughQuad / 2), wq(kRoughQuad / 2), q(2 * kRoughQuad);
        smrt_host::gauss_legendre_positive(kRoughQuad / 2, x.data(), wq.data());
        for (int a = 0; a < kRoughQuad / 2; ++a) {
            q[a] = 0.5 * (1.0 + x[a]); q[kRoughQuad / 2 + a] = 0.5 * (1.0 - x[a]);
            q[kRoughQuad + a] = q[kRoughQuad + kRoughQuad / 2 + a] = 0.5 * wq[a];
        }
        HIPCHK(st->quad.reserve(sizeof(double) * q.size()));
        HIPCHK(hipMemcpy(st->quad.p, q.data(), sizeof(double) * q.size(), hipMemcpyHostToDevice));
        st->quad_ready = true;
    }
    r.quad = (const double*)st->quad.p;
    const size_t np = (size_t)d.pair_count;
    HIPCHK(st->mu.reserve(sizeof(double) * np * W * nmax));
    HIPCHK(st->w.reserve(sizeof(double) * np * W * nmax));
    HIPCHK(st->n.reserve(sizeof(int) * np * W));
    HIPCHK(st->eps.reserve(sizeof(double) * np * L * 2));
    HIPCHK(hipMemsetAsync(st->n.p, 0, sizeof(int) * np * W, ctx->stream));
    r.ws_mu = (double*)st->mu.p; r.ws_w = (double*)st->w.p; r.ws_n = (int*)st->n.p; r.ws_eps = (double*)st->eps.p;
    size_t built = 0;
    if (slots > 0) {
        const size_t mat = sizeof(double) * FS * slots * nmodes * 4 * NE * NE, coh = sizeof(double) * FS * slots * 4 * NE;
        HIPCHK(ctx->d_itfslot.reserve(sizeof(int32_t) * FS * L));
        HIPCHK(ctx->d_itf.reserve(mat));
        HIPCHK(ctx->d_itfcoh.reserve(coh));
        HIPCHK(hipMemsetAsync(ctx->d_itfslot.p, 0xFF, sizeof(int32_t) * FS * L, ctx->stream));   // -1: Flat
        HIPCHK(hipMemsetAsync(ctx->d_itf.p, 0, mat, ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->d_itfcoh.p, 0, coh, ctx->stream));
        r.itf_slot = (int*)ctx->d_itfslot.p; r.itf = (double*)ctx->d_itf.p; r.itf_coh = (double*)ctx->d_itfcoh.p;
        d.host_itf_slot = r.itf_slot; d.host_itf = r.itf; d.host_itf_coh = r.itf_coh; d.host_itf_slots = slots;
        built += mat + coh;
    }
    if (has_sub) {   // the substrate's permittivity stays with the builder; the solve reads the dense matrices (SUB_HOST)
        const size_t mat = sizeof(double) * FS * nmodes * NE * NE, coh = sizeof(double) * FS * nmodes * NE;
        HIPCHK(st->sub1.reserve(sizeof(double) * FS));
        HIPCHK(st->sub2.reserve(sizeof(double) * FS));
        HIPCHK(hipMemcpyAsync(st->sub1.p, b->substrate_p1, sizeof(double) * FS, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(st->sub2.p, b->substrate_p2, sizeof(double) * FS, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx->d_sub1.reserve(mat));
        HIPCHK(ctx->d_sub2.reserve(coh));
        HIPCHK(hipMemsetAsync(ctx->d_sub1.p, 0, mat, ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->d_sub2.p, 0, coh, ctx->stream));
        r.sub_p1 = (const double*)st->sub1.p; r.sub_p2 = (const double*)st->sub2.p;
        r.sub = (double*)ctx->d_sub1.p; r.sub_coh = (double*)ctx->d_sub2.p;
        d.sub_kind = SUB_HOST; d.host_substrate = r.sub; d.host_substrate_coh = r.sub_coh;
        built += mat + coh;
    }
    const long long nb = slots + has_sub, tasks = (long long)np * nb, tiles = ((long long)nmax * nmax + kRoughNT - 1) / kRoughNT;
    const long long go_blocks = tasks * 4 * tiles, diag_blocks = (tasks * 4 * nmax + kRoughNT - 1) / kRoughNT, hemi_blocks = tasks * 2 * nmax;
    if (go_blocks > INT_MAX || hemi_blocks > INT_MAX) { ctx->err = "too many rough boundaries for one launch: split the batch"; return -1; }
    st->rewind();
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(rough_setup_kernel, dim3((unsigned)np), dim3(kRoughNT), 0, ctx->stream, r);
    HIPCHK(hipGetLastError());
    bool go = false, diag = false, hemi = false;   // which kernels the kinds of this batch need
    for (size_t i = 0; i < (size_t)S * W; ++i) {
        go |= b->rough_kind[i] == SMRT_ROUGH_GEOMETRICAL_OPTICS;
        diag |= b->rough_kind[i] == SMRT_ROUGH_IEM_FUNG92 || b->rough_kind[i] == SMRT_ROUGH_GEOMETRICAL_OPTICS_BACKSCATTER;
        hemi |= b->rough_kind[i] == SMRT_ROUGH_GEOMETRICAL_OPTICS_BACKSCATTER;
    }
    if (go && tasks > 0) {
        void (*kern)(RoughBatch) = nmodes == 1 ? rough_go_kernel<1> : nmodes == 2 ? rough_go_kernel<2> : nmodes == 3 ? rough_go_kernel<3>
                                 : nmodes == 4 ? rough_go_kernel<4> : rough_go_kernel<5>;
        hipLaunchKernelGGL(kern, dim3((unsigned)go_blocks), dim3(kRoughNT), 0, ctx->stream, r);
        HIPCHK(hipGetLastError());
    }
    if (diag && tasks > 0) {
        hipLaunchKernelGGL(rough_diag_kernel, dim3((unsigned)diag_blocks), dim3(kRoughNT), 0, ctx->stream, r);
        HIPCHK(hipGetLastError());
    }
    if (hemi && tasks > 0) {
        hipLaunchKernelGGL(rough_hemi_kernel, dim3((unsigned)hemi_blocks), dim3(kRoughNT), 0, ctx->stream, r);
        HIPCHK(hipGetLastError());
    }
    if (solver_host::record(ctx, st)) return -1;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, st->ev[0], st->ev[1]));
    ctx->rough_info.slots = slots; ctx->rough_info.has_sub = has_sub; ctx->rough_info.ms = ms; ctx->rough_info.built_bytes = built;
    return 0;
}

}  // namespace smrt_launch
