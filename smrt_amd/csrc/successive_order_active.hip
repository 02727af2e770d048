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

#include "solver_describe.hpp"
#include "solver_host.hpp"
#include "solver_refusals.hpp"

using namespace smrt;

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

struct SuccessiveOrderActiveState : solver_host::InputState {
    DevBuf &theta = buf(), &gl = buf();
    DevBuf &stage = buf(), &nsub = buf(), &nstream = buf(), &vec = buf(), &air = buf(), &wsoff = buf(), &chunk = buf(), &out = buf(),
           &status = buf(), &layer = buf(), &streams = buf(), &maxrad = buf(), &orders = buf(), &back = buf(), &inc = buf();
    SoaBatch dev{};
    bool uploaded = false, launched = false;
    int64_t budget = 0;
    size_t fixed_bytes = 0;             // everything reserved but the chunk buffer
    size_t chunk_bytes = 0;             // the chunk buffer (Wt + workspace of the largest chunk)
    std::vector<int32_t> nsub_host;     // [n_pairs][Lmax] after a launch
    std::vector<long long> deep;        // rows that do not fit the budget
    int64_t n_chunks = 0;               // events 0, 1: layers kernel; then four per chunk
};

constexpr int64_t kSoaDefaultBudget = 8LL << 30;

namespace smrt_launch {
void successive_order_active_release(smrt_dort_ctx* ctx) { solver_host::release(ctx->successive_order_active); }
}  // namespace smrt_launch

extern "C" {

int32_t smrt_so_active_out_stride(int32_t n_theta_inc, int32_t n_iteration_max) {
    return (n_theta_inc >= 1 && n_iteration_max >= 1) ? 9 * n_theta_inc * (n_iteration_max + 1) : -1;
}

int32_t smrt_so_active_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, int32_t n_iteration_max,
                                                  double relative_tolerance, int32_t n_theta_inc, const double* theta_inc,
                                                  int32_t incident_npol, int32_t m_max, int64_t workspace_budget_bytes,
                                                  const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = solver_refusals::successive_order_active(b, n_iteration_max, relative_tolerance, n_theta_inc, theta_inc, incident_npol, m_max);
    if (why) { ctx->err = why; return -1; }
    if (solver_host::check_pairs(ctx, pairs, &n_pairs, (int64_t)b->n_snowpacks * b->n_frequencies)) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->successive_order_active) ctx->successive_order_active = new SuccessiveOrderActiveState();
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    st->uploaded = st->launched = false;
    st->budget = workspace_budget_bytes > 0 ? workspace_budget_bytes : kSoaDefaultBudget;
    SoaBatch a = solver_describe::successive_order_active(b, n_iteration_max, relative_tolerance, n_theta_inc, incident_npol, m_max, n_pairs);
    SoBatch& d = a.so;
    const solver_describe::SoaExtents n = solver_describe::extents(a);
    // everything but the chunk buffer, counted before anything is reserved: the budget is checked first
    const size_t out_bytes[] = {n.stage * 8, n.nsub * 4, n.nstream * 4, n.vec * 8, n.air * 8, n.ws_off * 8,
                                n.out * 8, n.status * 4, n.layer_out * 8, n.streams * 8, n.maxrad * 8, n.orders * 4,
                                n.back * 8, n.inc * 4};
    size_t fixed = solver_describe::input_bytes(b, solver_describe::inputs(d, pairs != nullptr)) + (n.theta + n.gl_mu) * 8;
    for (size_t v : out_bytes) fixed += v;
    if ((int64_t)fixed >= st->budget) {
        ctx->err = "the workspace budget of the successive_order_backscatter solver is smaller than the buffers of the batch itself (" +
                   std::to_string(fixed) + " bytes)";
        return -1;
    }
    using solver_host::upload;
    if (solver_host::upload_batch(ctx, st, b, pairs, d)) return -1;
    if (upload(ctx, st->theta, theta_inc, n.theta * sizeof(double), d.theta)) return -1;
    std::vector<double> gl(n.gl_mu);
    smrt_host::gauss_legendre_positive(d.nmax, gl.data(), nullptr);
    if (upload(ctx, st->gl, gl.data(), n.gl_mu * sizeof(double), d.gl_mu)) return -1;
    DevBuf* outs[] = {&st->stage, &st->nsub, &st->nstream, &st->vec, &st->air, &st->wsoff, &st->out, &st->status, &st->layer,
                      &st->streams, &st->maxrad, &st->orders, &st->back, &st->inc};
    for (size_t k = 0; k < sizeof(outs) / sizeof(outs[0]); ++k) HIPCHK(outs[k]->reserve(out_bytes[k]));
    d.stage = (double*)st->stage.p; d.nsub = (int*)st->nsub.p; d.nstream = (int*)st->nstream.p; d.vec = (double*)st->vec.p;
    a.air = (double*)st->air.p; d.ws_off = (const long long*)st->wsoff.p; d.out = (double*)st->out.p;
    d.status = (int*)st->status.p; d.layer_out = (double*)st->layer.p; d.streams = (double*)st->streams.p;
    d.maxrad = (double*)st->maxrad.p; d.orders = (int*)st->orders.p; a.back = (double*)st->back.p; a.inc = (int*)st->inc.p;
    if (solver_host::uploads_done(ctx)) return -1;
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
    st->rewind();
    st->deep.clear();
    // (a) layer scalars and sublayer counts; the counts come back: they size the workspace
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(successive_order_active_layers_kernel, dim3((unsigned)((N * L + kSoaThreads - 1) / kSoaThreads)), dim3(kSoaThreads), 0,
                       ctx->stream, a);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    st->nsub_host.resize((size_t)(N * L));
    HIPCHK(hipMemcpyAsync(st->nsub_host.data(), d.nsub, (size_t)(N * L) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // the chunk plan: consecutive rows whose Wt matrices ((m_max + 1) x Lmax x Dp^2 per pair) and workspaces ((m_max + 2) passes
    // per pair, sized for the largest column count) fit what the budget leaves
    const solver_describe::SoaExtents n = solver_describe::extents(a);
    const long long wt_pair = (long long)n.wt_pair;              // doubles
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
    const size_t lds = n.lds_sweep;
    const long long row = 9LL * d.n_theta * (d.n_iter + 1);
    for (size_t c = 0; c < begin.size(); ++c) {
        d.chunk_begin = begin[c]; d.chunk_count = count[c];
        d.wt = (double*)st->chunk.p;
        d.ws = d.wt + count[c] * wt_pair;
        if (solver_host::record(ctx, st)) return -1;
        hipLaunchKernelGGL(successive_order_active_prep_kernel, dim3((unsigned)(count[c] * L * M)), dim3(kSoaThreads), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        if (solver_host::record(ctx, st)) return -1;
        hipLaunchKernelGGL(successive_order_active_sweep_kernel, dim3((unsigned)(count[c] * NP)), dim3(kSoaThreads), lds, ctx->stream, a);
        HIPCHK(hipGetLastError());
        if (solver_host::record(ctx, st)) return -1;
        hipLaunchKernelGGL(successive_order_active_combine_kernel, dim3((unsigned)((count[c] * row + kSoaThreads - 1) / kSoaThreads)),
                           dim3(kSoaThreads), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        if (solver_host::record(ctx, st)) return -1;
    }
    st->launched = true;
    return 0;
}

int32_t smrt_so_active_sync(smrt_dort_ctx* ctx) { return solver_host::sync(ctx); }

int32_t smrt_so_active_kernel_ms(smrt_dort_ctx* ctx, double* ms3) {
    if (!ctx || !ms3) return -1;
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    if (!st || !st->launched) { ctx->err = "no successive-order backscatter launch to time"; return -1; }
    double prep = 0.0, sweep = 0.0, combine = 0.0;
    if (solver_host::wait_recorded(ctx, st) || solver_host::add_elapsed(ctx, st, 0, 1, &prep)) return -1;
    for (size_t k = 2; k + 3 < st->ev_used; k += 4)
        if (solver_host::add_elapsed(ctx, st, k, k + 1, &prep) || solver_host::add_elapsed(ctx, st, k + 1, k + 2, &sweep) ||
            solver_host::add_elapsed(ctx, st, k + 2, k + 3, &combine))
            return -1;
    ms3[0] = prep; ms3[1] = sweep; ms3[2] = combine;
    return 0;
}

int32_t smrt_so_active_launch_info(smrt_dort_ctx* ctx, int64_t* info, int32_t capacity) {
    if (!ctx) return -1;
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    if (!st || !st->launched) { ctx->err = "no successive-order backscatter launch to describe"; return -1; }
    const int64_t v[] = {st->n_chunks, (int64_t)(st->fixed_bytes + st->chunk_bytes), (int64_t)st->deep.size(), st->budget};
    return solver_host::copy_table(v, info, capacity);
}

int32_t smrt_so_active_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* streams,
                                              int32_t* sublayers, double* max_radiance, int32_t* orders) {
    if (!ctx) return -1;
    SuccessiveOrderActiveState* st = ctx->successive_order_active;
    if (!st || !st->launched) { ctx->err = "no successive-order backscatter launch to download"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const SoBatch& d = st->dev.so;
    const solver_describe::SoaExtents n = solver_describe::extents(st->dev);
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, n.out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, n.status * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.layer_out, n.layer_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (streams) HIPCHK(hipMemcpyAsync(streams, d.streams, n.streams * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (max_radiance) HIPCHK(hipMemcpyAsync(max_radiance, d.maxrad, n.maxrad * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (orders) HIPCHK(hipMemcpyAsync(orders, d.orders, n.orders * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (sublayers) std::memcpy(sublayers, st->nsub_host.data(), n.nsub * sizeof(int32_t));
    for (long long i : st->deep) {   // the rows no kernel touched
        const size_t N = (size_t)d.n_pairs, row = n.out / N, NS = n.streams / N, NO = n.maxrad / N, NP = n.orders / N;   // per pair
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
