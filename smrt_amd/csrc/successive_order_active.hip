// The successive-order backscatter solver of libsmrt_dort.so (include/smrt_dort.h: smrt_so_active_*): its
// kernels -- one lane per (pair, layer) for the layer electromagnetics (the passive solver's so_layer_item), one workgroup
// per (pair, layer, mode) for the interface coefficients and the weighted phase matrices, one workgroup per (pair, pass) for
// all the orders, one lane per output element for the combination; arithmetic in successive_order_active_kernel.hpp -- and
// the host side: buffers on the DORT context, the chunk plan that keeps everything inside one budget, upload / launch /
// sync / download and the one-shot call.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "dort_ctx.hpp"
#include "dort_host_common.hpp"
#include "successive_order_active_kernel.hpp"
#include "../../include/smrt_dort.h"

using namespace smrt;

#define HIPCHK(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
            return -1;                                                                            \
        }                                                                                         \
    } while (0)

__global__ void __launch_bounds__(kSoaThreads) successive_order_active_layers_kernel(SoaBatch a) {
    const long long idx = (long long)blockIdx.x * kSoaThreads + threadIdx.x;
    if (idx >= a.so.n_pairs * a.so.Lmax) return;
    so_layer_item(a.so, idx % a.so.n_pairs, (int)(idx / a.so.n_pairs));   // pairs fastest: the staging rows are written with unit stride
}

__global__ void __launch_bounds__(kSoaThreads) successive_order_active_prep_kernel(SoaBatch a) {
    const long long item = blockIdx.x;   // layers fastest, then modes: the Wt matrices of a pair are written next to each other
    const int M = a.m_max + 1;
    soa_prep_item<kSoaThreads>(a, a.so.chunk_begin + item / ((long long)a.so.Lmax * M), (int)(item % a.so.Lmax), (int)((item / a.so.Lmax) % M));
}

__global__ void __launch_bounds__(kSoaThreads) successive_order_active_sweep_kernel(SoaBatch a) {
    extern __shared__ double soa_lds[];
    const int NP = a.m_max + 2;
    soa_sweep_pass<kSoaThreads>(a, a.so.chunk_begin + blockIdx.x / NP, (int)(blockIdx.x % NP), soa_lds);
}

__global__ void __launch_bounds__(kSoaThreads) successive_order_active_combine_kernel(SoaBatch a) {
    const long long idx = (long long)blockIdx.x * kSoaThreads + threadIdx.x;
    const long long row = 9LL * a.so.n_theta * (a.so.n_iter + 1);
    if (idx >= a.so.chunk_count * row) return;
    soa_combine_item(a, a.so.chunk_begin + idx / row, (int)(idx % row));
}

struct SuccessiveOrderActiveState {
    DevBuf nl, thick, fv, temp, p1, p2, freq, theta, lw, kind, sub1, sub2, gl, pairmap;
    DevBuf stage, nsub, nstream, vec, air, wsoff, chunk, out, status, layer, streams, maxrad, orders, back, inc;
    SoaBatch dev{};
    bool uploaded = false, launched = false;
    int64_t budget = 0;
    size_t fixed_bytes = 0;             // everything reserved but the chunk buffer
    size_t chunk_bytes = 0;             // the chunk buffer (Wt + workspace of the largest chunk)
    std::vector<int32_t> nsub_host;     // [n_pairs][Lmax] after a launch
    std::vector<long long> deep;        // rows that do not fit the budget
    int64_t n_chunks = 0;
    std::vector<hipEvent_t> ev;         // pool
    size_t ev_used = 0;                 // [0, 1]: layers kernel; then four per chunk
};

constexpr int64_t kSoaDefaultBudget = 8LL << 30;

namespace smrt_launch {
void successive_order_active_release(smrt_dort_ctx* ctx) {
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    if (!st) return;
    DevBuf* bufs[] = {&st->nl, &st->thick, &st->fv, &st->temp, &st->p1, &st->p2, &st->freq, &st->theta, &st->lw, &st->kind, &st->sub1,
                      &st->sub2, &st->gl, &st->pairmap, &st->stage, &st->nsub, &st->nstream, &st->vec, &st->air, &st->wsoff,
                      &st->chunk, &st->out, &st->status, &st->layer, &st->streams, &st->maxrad, &st->orders, &st->back, &st->inc};
    for (DevBuf* b : bufs) b->release();
    for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
    delete st;
    ctx->successive_order_active = nullptr;
}
}  // namespace smrt_launch

static const char* soa_validate(const smrt_batch* b, int32_t n_iter, double rtol, int32_t n_theta_inc, const double* theta_inc,
                                int32_t incident_npol, int32_t m_max) {
    if (!b) return "null batch";
    if (b->n_snowpacks <= 0 || b->n_frequencies <= 0 || b->n_layers_max <= 0) return "empty batch";
    if (n_theta_inc <= 0 || !theta_inc) return "n_theta_inc must be positive";
    if (b->mode != SMRT_MODE_ACTIVE) return "the successive_order_backscatter solver needs an active sensor";
    if (n_iter < 1) return "n_iteration_max must be at least 1";
    if (!(rtol >= 0.0)) return "relative_tolerance must be non-negative";
    if (incident_npol < 1 || incident_npol > 3) return "incident_npol must be 1 (V), 2 (VH) or 3 (VHU)";
    if (b->n_max_stream < 2 || b->n_max_stream > kSoMaxStream) return "the successive_order_backscatter solver takes 2 to 64 streams";
    if (m_max < 0 || m_max > 64) return "m_max must be 0 to 64";
    if (b->emmodel < SMRT_EM_IBA || b->emmodel > SMRT_EM_RAYLEIGH_HOST) return "unknown emmodel";
    if (b->microstructure < SMRT_MS_EXPONENTIAL || b->microstructure > SMRT_MS_TEUBNER_STREY) return "unknown microstructure";
    if (!b->n_layers || !b->thickness || !b->frac_volume || !b->temperature || !b->micro_p1 || !b->frequency) return "null input array";
    if ((b->microstructure == SMRT_MS_STICKY_HARD_SPHERES || b->layer_kind) && !b->micro_p2) return "stickiness array missing";
    const char* host = "the successive_order_backscatter solver has no route for emmodels evaluated on the host";
    const char* shs = "the dmrt short-range emmodels are only compatible with sticky_hard_spheres";
    const char* rayleigh = "the Rayleigh-family emmodels have azimuth modes 0 to 2 only: m_max must be at most 2";
    if (!b->layer_kind) {
        if (b->emmodel == SMRT_EM_HOST || b->emmodel == SMRT_EM_IBA_HOST || b->emmodel == SMRT_EM_RAYLEIGH_HOST) return host;
        const bool dmrt = b->emmodel == SMRT_EM_DMRT_QCA_SHORTRANGE || b->emmodel == SMRT_EM_DMRT_QCACP_SHORTRANGE;
        if (dmrt && b->microstructure != SMRT_MS_STICKY_HARD_SPHERES) return shs;
        if (dmrt && m_max > 2) return rayleigh;
    }
    for (int s = 0; s < b->n_snowpacks; ++s) {
        if (b->n_layers[s] < 1 || b->n_layers[s] > b->n_layers_max) return "n_layers out of range";
        for (int l = 0; b->layer_kind && l < b->n_layers[s]; ++l) {
            const int k = b->layer_kind[(long long)s * b->n_layers_max + l], em = k & 15, ms = k >> 4;
            if (em < SMRT_EM_IBA || em > SMRT_EM_RAYLEIGH_HOST || ms < SMRT_MS_EXPONENTIAL || ms > SMRT_MS_TEUBNER_STREY)
                return "invalid layer_kind entry";
            if (em == SMRT_EM_HOST || em == SMRT_EM_IBA_HOST || em == SMRT_EM_RAYLEIGH_HOST) return host;
            const bool dmrt = em == SMRT_EM_DMRT_QCA_SHORTRANGE || em == SMRT_EM_DMRT_QCACP_SHORTRANGE;
            if (dmrt && ms != SMRT_MS_STICKY_HARD_SPHERES) return shs;
            if (dmrt && m_max > 2) return rayleigh;
        }
    }
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE && b->substrate_kind != SMRT_SUBSTRATE_FLAT)
        return "the successive_order_backscatter solver takes no substrate or a flat one (a reflector has no third Stokes component)";
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE && (!b->substrate_p1 || !b->substrate_p2)) return "substrate arrays missing";
    if (b->host_interface_slot) return "the successive_order_backscatter solver takes flat interfaces only";
    if (b->process_coherent_layers) return "the successive_order_backscatter solver does not process coherent layers";
    return nullptr;
}

static int soa_upload(smrt_dort_ctx* ctx, DevBuf& buf, const void* src, size_t bytes, size_t* total) {
    HIPCHK(buf.reserve(bytes));
    HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    *total += bytes;
    return 0;
}

static int soa_event(smrt_dort_ctx* ctx, SuccessiveOrderActiveState* st) {
    if (st->ev_used == st->ev.size()) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        st->ev.push_back(e);
    }
    HIPCHK(hipEventRecord(st->ev[st->ev_used++], ctx->stream));
    return 0;
}

extern "C" {

int32_t smrt_so_active_out_stride(int32_t n_theta_inc, int32_t n_iteration_max) {
    return (n_theta_inc >= 1 && n_iteration_max >= 1) ? 9 * n_theta_inc * (n_iteration_max + 1) : -1;
}

int32_t smrt_so_active_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, int32_t n_iteration_max,
                                                  double relative_tolerance, int32_t n_theta_inc, const double* theta_inc,
                                                  int32_t incident_npol, int32_t m_max, int64_t workspace_budget_bytes,
                                                  const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = soa_validate(b, n_iteration_max, relative_tolerance, n_theta_inc, theta_inc, incident_npol, m_max);
    if (why) { ctx->err = why; return -1; }
    const int64_t all = (int64_t)b->n_snowpacks * b->n_frequencies;
    if (!pairs) n_pairs = all;
    else {
        if (n_pairs <= 0) { ctx->err = "empty pair list"; return -1; }
        for (int64_t i = 0; i < n_pairs; ++i)
            if (pairs[i] < 0 || pairs[i] >= all) { ctx->err = "pair index out of bounds"; return -1; }
    }
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->successive_order_active) ctx->successive_order_active = new SuccessiveOrderActiveState();
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    st->uploaded = st->launched = false;
    st->budget = workspace_budget_bytes > 0 ? workspace_budget_bytes : kSoaDefaultBudget;
    const size_t S = b->n_snowpacks, L = b->n_layers_max, F = b->n_frequencies, T = n_theta_inc, N = (size_t)n_pairs;
    const size_t SL = S * L * sizeof(double), FS = F * S, NM = b->n_max_stream, NO = n_iteration_max, NP = m_max + 2;
    const size_t Dh = 3 * NM, CM = soa_max_columns(incident_npol, n_theta_inc, (int)NM);
    // everything but the chunk buffer, counted before anything is reserved: the budget is checked first
    const size_t out_bytes[] = {(size_t)SO_ROWS * L * N * 8, N * L * 4, N * L * 4, N * L * SOA_VECS * Dh * 8, N * 2 * Dh * 8, N * 8,
                                N * 9 * T * (NO + 1) * 8, N * 4, N * L * 5 * 8, N * (1 + NM) * 8, N * NP * NO * 8, N * NP * 4,
                                N * NP * NO * 3 * CM * 8, N * (1 + NM) * 4};
    size_t fixed = S * 4 + 5 * SL + (b->liquid_water ? SL : 0) + (b->layer_kind ? S * L * 4 : 0) + F * 8 + T * 8 + NM * 8 +
                   (b->substrate_kind != SMRT_SUBSTRATE_NONE ? 2 * FS * 8 : 0) + (pairs ? N * 8 : 0);
    for (size_t v : out_bytes) fixed += v;
    if ((int64_t)fixed >= st->budget) {
        ctx->err = "the workspace budget of the successive_order_backscatter solver is smaller than the buffers of the batch itself (" +
                   std::to_string(fixed) + " bytes)";
        return -1;
    }
    SoaBatch a{};
    SoBatch& d = a.so;
    d.S = (int)S; d.Lmax = (int)L; d.F = (int)F; d.n_theta = (int)T;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.sub_kind = b->substrate_kind; d.nmax = (int)NM;
    d.n_iter = n_iteration_max; d.rj = 0; d.nsamp = azimuth_samples(m_max);
    d.rtol = relative_tolerance;
    d.n_pairs = n_pairs;
    a.npi = incident_npol; a.m_max = m_max; a.Cmax = (int)CM; a.phi = b->phi;
    size_t up = 0;
#define SO_UP(buf, src, bytes, field) do { if (soa_upload(ctx, st->buf, src, bytes, &up)) return -1; d.field = (decltype(d.field))st->buf.p; } while (0)
    SO_UP(nl, b->n_layers, S * sizeof(int32_t), n_layers);
    SO_UP(thick, b->thickness, SL, thickness);
    SO_UP(fv, b->frac_volume, SL, frac_volume);
    SO_UP(temp, b->temperature, SL, temperature);
    SO_UP(p1, b->micro_p1, SL, p1);
    if (b->micro_p2) SO_UP(p2, b->micro_p2, SL, p2);
    SO_UP(freq, b->frequency, F * sizeof(double), frequency);
    SO_UP(theta, theta_inc, T * sizeof(double), theta);
    if (b->liquid_water) SO_UP(lw, b->liquid_water, SL, liquid_water);
    if (b->layer_kind) SO_UP(kind, b->layer_kind, S * L * sizeof(int32_t), layer_kind);
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE) {
        SO_UP(sub1, b->substrate_p1, FS * sizeof(double), sub_p1);
        SO_UP(sub2, b->substrate_p2, FS * sizeof(double), sub_p2);
    }
    std::vector<double> gl(NM);
    smrt_host::gauss_legendre_positive((int)NM, gl.data(), nullptr);
    SO_UP(gl, gl.data(), NM * sizeof(double), gl_mu);
    if (pairs) SO_UP(pairmap, pairs, N * sizeof(int64_t), pair_map);
#undef SO_UP
    DevBuf* outs[] = {&st->stage, &st->nsub, &st->nstream, &st->vec, &st->air, &st->wsoff, &st->out, &st->status, &st->layer,
                      &st->streams, &st->maxrad, &st->orders, &st->back, &st->inc};
    for (size_t k = 0; k < sizeof(outs) / sizeof(outs[0]); ++k) HIPCHK(outs[k]->reserve(out_bytes[k]));
    d.stage = (double*)st->stage.p; d.nsub = (int*)st->nsub.p; d.nstream = (int*)st->nstream.p; d.vec = (double*)st->vec.p;
    a.air = (double*)st->air.p; d.ws_off = (const long long*)st->wsoff.p; d.out = (double*)st->out.p;
    d.status = (int*)st->status.p; d.layer_out = (double*)st->layer.p; d.streams = (double*)st->streams.p;
    d.maxrad = (double*)st->maxrad.p; d.orders = (int*)st->orders.p; a.back = (double*)st->back.p; a.inc = (int*)st->inc.p;
    // the copies above read the caller's (pageable) arrays and this function's own vectors: wait for them
    HIPCHK(hipStreamSynchronize(ctx->stream));
    st->fixed_bytes = fixed;
    st->dev = a;
    st->uploaded = true;
    return 0;
}

int32_t smrt_so_active_launch(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    if (!st || !st->uploaded) { ctx->err = "no successive-order backscatter batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    SoaBatch a = st->dev;
    SoBatch& d = a.so;
    const long long N = d.n_pairs, L = d.Lmax, M = a.m_max + 1, NP = a.m_max + 2;
    st->launched = false;
    st->ev_used = 0;
    st->deep.clear();
    // (a) layer scalars and sublayer counts; the counts come back: they size the workspace
    if (soa_event(ctx, st)) return -1;
    hipLaunchKernelGGL(successive_order_active_layers_kernel, dim3((unsigned)((N * L + kSoaThreads - 1) / kSoaThreads)), dim3(kSoaThreads), 0,
                       ctx->stream, a);
    HIPCHK(hipGetLastError());
    if (soa_event(ctx, st)) return -1;
    st->nsub_host.resize((size_t)(N * L));
    HIPCHK(hipMemcpyAsync(st->nsub_host.data(), d.nsub, (size_t)(N * L) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // the chunk plan: consecutive rows whose Wt matrices ((m_max + 1) x Lmax x Dp^2 per pair) and workspaces ((m_max + 2) passes
    // per pair, sized for the largest column count) fit what the budget leaves
    const long long Dp = soa_dp(d.nmax);
    const long long wt_pair = M * L * Dp * Dp;                   // doubles
    const long long avail = (st->budget - (int64_t)st->fixed_bytes) / 8;   // doubles
    std::vector<long long> ws_off((size_t)N, 0), begin, count;
    long long cur_ws = 0, cur_n = 0, cur_begin = 0, largest = 0;
    auto close = [&](long long next_begin) {
        if (cur_n > 0) {
            begin.push_back(cur_begin); count.push_back(cur_n);
            if (cur_n * wt_pair + cur_ws > largest) largest = cur_n * wt_pair + cur_ws;
        }
        cur_begin = next_begin; cur_n = 0; cur_ws = 0;
    };
    for (long long i = 0; i < N; ++i) {
        long long n_sub = 0, n_lay = 0;
        for (long long l = 0; l < L; ++l) { const int k = st->nsub_host[(size_t)(i * L + l)]; n_sub += k; n_lay += k > 0; }
        const long long ws = NP * soa_pass_doubles(n_sub, n_lay, a.Cmax, d.nmax);
        if (wt_pair + ws > avail) { close(i + 1); st->deep.push_back(i); continue; }
        if ((cur_n + 1) * wt_pair + cur_ws + ws > avail) close(i);
        ws_off[(size_t)i] = cur_ws;
        cur_ws += ws; ++cur_n;
    }
    close(N);
    st->n_chunks = (int64_t)begin.size();
    st->chunk_bytes = (size_t)largest * 8;
    if (largest > 0) HIPCHK(st->chunk.reserve((size_t)largest * 8));
    HIPCHK(hipMemcpyAsync(st->wsoff.p, ws_off.data(), (size_t)N * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (ws_off is a local vector)
    const size_t lds = (size_t)soa_lds_doubles(d.nmax) * sizeof(double);
    const long long row = 9LL * d.n_theta * (d.n_iter + 1);
    for (size_t c = 0; c < begin.size(); ++c) {
        d.chunk_begin = begin[c]; d.chunk_count = count[c];
        d.wt = (double*)st->chunk.p;
        d.ws = d.wt + count[c] * wt_pair;
        if (soa_event(ctx, st)) return -1;
        hipLaunchKernelGGL(successive_order_active_prep_kernel, dim3((unsigned)(count[c] * L * M)), dim3(kSoaThreads), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        if (soa_event(ctx, st)) return -1;
        hipLaunchKernelGGL(successive_order_active_sweep_kernel, dim3((unsigned)(count[c] * NP)), dim3(kSoaThreads), lds, ctx->stream, a);
        HIPCHK(hipGetLastError());
        if (soa_event(ctx, st)) return -1;
        hipLaunchKernelGGL(successive_order_active_combine_kernel, dim3((unsigned)((count[c] * row + kSoaThreads - 1) / kSoaThreads)),
                           dim3(kSoaThreads), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        if (soa_event(ctx, st)) return -1;
    }
    st->launched = true;
    return 0;
}

int32_t smrt_so_active_sync(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_so_active_kernel_ms(smrt_dort_ctx* ctx, double* ms3) {
    if (!ctx || !ms3) return -1;
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    if (!st || !st->launched) { ctx->err = "no successive-order backscatter launch to time"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(st->ev[st->ev_used - 1]));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, st->ev[0], st->ev[1]));
    double prep = f, sweep = 0.0, combine = 0.0;
    for (size_t k = 2; k + 3 < st->ev_used; k += 4) {
        HIPCHK(hipEventElapsedTime(&f, st->ev[k], st->ev[k + 1]));
        prep += f;
        HIPCHK(hipEventElapsedTime(&f, st->ev[k + 1], st->ev[k + 2]));
        sweep += f;
        HIPCHK(hipEventElapsedTime(&f, st->ev[k + 2], st->ev[k + 3]));
        combine += f;
    }
    ms3[0] = prep; ms3[1] = sweep; ms3[2] = combine;
    return 0;
}

int32_t smrt_so_active_launch_info(smrt_dort_ctx* ctx, int64_t* info, int32_t capacity) {
    if (!ctx) return -1;
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    if (!st || !st->launched) { ctx->err = "no successive-order backscatter launch to describe"; return -1; }
    const int64_t v[] = {st->n_chunks, (int64_t)(st->fixed_bytes + st->chunk_bytes), (int64_t)st->deep.size(), st->budget};
    const int32_t n = (int32_t)(sizeof(v) / sizeof(v[0]));
    for (int32_t i = 0; info && i < n && i < capacity; ++i) info[i] = v[i];
    return n;
}

int32_t smrt_so_active_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* streams,
                                              int32_t* sublayers, double* max_radiance, int32_t* orders) {
    if (!ctx) return -1;
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    if (!st || !st->launched) { ctx->err = "no successive-order backscatter launch to download"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const SoBatch& d = st->dev.so;
    const size_t N = (size_t)d.n_pairs, L = d.Lmax, row = (size_t)9 * d.n_theta * (d.n_iter + 1), NS = 1 + d.nmax;
    const size_t NP = st->dev.m_max + 2, NO = NP * d.n_iter;
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, N * row * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, N * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.layer_out, N * L * 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (streams) HIPCHK(hipMemcpyAsync(streams, d.streams, N * NS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (max_radiance) HIPCHK(hipMemcpyAsync(max_radiance, d.maxrad, N * NO * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (orders) HIPCHK(hipMemcpyAsync(orders, d.orders, N * NP * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (sublayers) std::memcpy(sublayers, st->nsub_host.data(), N * L * sizeof(int32_t));
    for (long long i : st->deep) {   // the rows no kernel touched
        if (out) for (size_t k = 0; k < row; ++k) out[(size_t)i * row + k] = NAN;
        if (status) status[i] = ST_DEPTH;
        if (streams) for (size_t k = 0; k < NS; ++k) streams[(size_t)i * NS + k] = 0.0;
        if (max_radiance) for (size_t k = 0; k < NO; ++k) max_radiance[(size_t)i * NO + k] = NAN;
        if (orders) for (size_t k = 0; k < NP; ++k) orders[(size_t)i * NP + k] = 0;
    }
    return 0;
}

int32_t smrt_so_active_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, int32_t n_iteration_max,
                                               double relative_tolerance, int32_t n_theta_inc, const double* theta_inc,
                                               int32_t incident_npol, int32_t m_max, int64_t workspace_budget_bytes,
                                               const int64_t* pairs, int64_t n_pairs, double* out, int32_t* status, double* layer_out,
                                               double* streams, int32_t* sublayers, double* max_radiance, int32_t* orders) {
    if (smrt_so_active_upload_pairs(ctx, batch, n_iteration_max, relative_tolerance, n_theta_inc, theta_inc,
                                                  incident_npol, m_max, workspace_budget_bytes, pairs, n_pairs))
        return -1;
    if (smrt_so_active_launch(ctx)) return -1;
    return smrt_so_active_download(ctx, out, status, layer_out, streams, sublayers, max_radiance, orders);
}

}  // extern "C"
