// The multi-Fresnel thermal emission solver of libsmrt_dort.so (include/smrt_dort.h: smrt_multifresnel_*): its two kernels --
// one lane per (pair, layer slot) for the layer electromagnetics, one lane per (pair, sensor angle) for the chain of layer
// matrices; arithmetic in multifresnel_kernel.hpp -- and the host side: buffers on the DORT context, upload / launch / sync /
// download and the one-shot call.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <string>

#include "solver_describe.hpp"
#include "solver_host.hpp"
#include "solver_refusals.hpp"

using namespace smrt;

constexpr int kMfThreads = 256;

__global__ void __launch_bounds__(kMfThreads) multifresnel_layers_kernel(MfBatch b) {
    const long long idx = (long long)blockIdx.x * kMfThreads + threadIdx.x;
    if (idx >= b.n_pairs * (b.Lmax + 1)) return;
    multifresnel_layer_item(b, idx % b.n_pairs, (int)(idx / b.n_pairs));   // pairs fastest: the staging rows are written with unit stride
}

__global__ void __launch_bounds__(kMfThreads) multifresnel_chain_kernel(MfBatch b) {
    const long long idx = (long long)blockIdx.x * kMfThreads + threadIdx.x;
    if (idx >= b.n_pairs * b.n_theta) return;
    multifresnel_chain_item(b, idx / b.n_theta, (int)(idx % b.n_theta));   // angles fastest: a wavefront reads 64 / n_theta consecutive staging entries per row
}

struct MultiFresnelState : solver_host::InputState {
    DevBuf &mu = buf(), &subT = buf();
    DevBuf &stage = buf(), &out = buf(), &status = buf(), &used = buf(), &tau = buf(), &layer = buf();
    MfBatch dev{};
    bool uploaded = false;
    bool timed = false;   // events 0, 1, 2 around the two kernels of the last launch
};

namespace smrt_launch {
void multifresnel_release(smrt_dort_ctx* ctx) { solver_host::release(ctx->multifresnel); }
}  // namespace smrt_launch

extern "C" {

int32_t smrt_multifresnel_out_stride(const smrt_batch* b) { return b ? 2 * b->n_theta : -1; }

int32_t smrt_multifresnel_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const double* mu, double prune_deep_snowpack,
                                       int32_t prune_none, const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = solver_refusals::multifresnel(b, mu, prune_deep_snowpack, prune_none);
    if (why) { ctx->err = why; return -1; }
    if (solver_host::check_pairs(ctx, pairs, &n_pairs, (int64_t)b->n_snowpacks * b->n_frequencies)) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->multifresnel) ctx->multifresnel = new MultiFresnelState();
    MultiFresnelState* st = ctx->multifresnel;
    st->uploaded = false;
    MfBatch d = solver_describe::multifresnel(b, mu, prune_deep_snowpack, prune_none, n_pairs);
    const solver_describe::MfExtents n = solver_describe::extents(d);
    if (solver_host::upload_batch(ctx, st, b, pairs, d)) return -1;
    if (solver_host::upload(ctx, st->mu, mu, n.mu * sizeof(double), d.mu)) return -1;
    if (b->substrate_kind == SMRT_SUBSTRATE_FLAT && solver_host::upload(ctx, st->subT, b->substrate_temperature, n.sub_T * sizeof(double), d.sub_T)) return -1;
    using solver_host::reserve;
    if (reserve(ctx, st->stage, n.stage, d.stage) || reserve(ctx, st->out, n.out, d.out) || reserve(ctx, st->status, n.status, d.status) ||
        reserve(ctx, st->used, n.layers_used, d.layers_used) || reserve(ctx, st->tau, n.tau_snowpack, d.tau_snowpack) ||
        reserve(ctx, st->layer, n.layer_out, d.layer_out) || solver_host::uploads_done(ctx))
        return -1;
    st->dev = d;
    st->uploaded = true;
    st->timed = false;
    return 0;
}

int32_t smrt_multifresnel_launch(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    MultiFresnelState* st = ctx->multifresnel;
    if (!st || !st->uploaded) { ctx->err = "no multi-Fresnel batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const MfBatch& d = st->dev;
    const long long items_a = d.n_pairs * (d.Lmax + 1), items_b = d.n_pairs * d.n_theta;
    st->rewind();
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(multifresnel_layers_kernel, dim3((unsigned)((items_a + kMfThreads - 1) / kMfThreads)), dim3(kMfThreads), 0,
                       ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(multifresnel_chain_kernel, dim3((unsigned)((items_b + kMfThreads - 1) / kMfThreads)), dim3(kMfThreads), 0,
                       ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    st->timed = true;
    return 0;
}

int32_t smrt_multifresnel_sync(smrt_dort_ctx* ctx) { return solver_host::sync(ctx); }

int32_t smrt_multifresnel_kernel_ms(smrt_dort_ctx* ctx, double* ms2) {
    if (!ctx || !ms2) return -1;
    MultiFresnelState* st = ctx->multifresnel;
    if (!st || !st->timed) { ctx->err = "no multi-Fresnel launch to time"; return -1; }
    ms2[0] = ms2[1] = 0.0;
    if (solver_host::wait_recorded(ctx, st) || solver_host::add_elapsed(ctx, st, 0, 1, &ms2[0]) || solver_host::add_elapsed(ctx, st, 1, 2, &ms2[1])) return -1;
    return 0;
}

int32_t smrt_multifresnel_download(smrt_dort_ctx* ctx, double* out, int32_t* status, int32_t* layers_used, double* tau_snowpack,
                                   double* layer_out) {
    if (!ctx) return -1;
    MultiFresnelState* st = ctx->multifresnel;
    if (!st || !st->uploaded) { ctx->err = "no multi-Fresnel batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const MfBatch& d = st->dev;
    const solver_describe::MfExtents n = solver_describe::extents(d);
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, n.out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, n.status * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (layers_used) HIPCHK(hipMemcpyAsync(layers_used, d.layers_used, n.layers_used * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (tau_snowpack) HIPCHK(hipMemcpyAsync(tau_snowpack, d.tau_snowpack, n.tau_snowpack * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.layer_out, n.layer_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_multifresnel_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const double* mu, double prune_deep_snowpack,
                                    int32_t prune_none, const int64_t* pairs, int64_t n_pairs, double* out, int32_t* status,
                                    int32_t* layers_used, double* tau_snowpack, double* layer_out) {
    if (smrt_multifresnel_upload_pairs(ctx, batch, mu, prune_deep_snowpack, prune_none, pairs, n_pairs)) return -1;
    if (smrt_multifresnel_launch(ctx)) return -1;
    return smrt_multifresnel_download(ctx, out, status, layers_used, tau_snowpack, layer_out);
}

}  // extern "C"
