// The multi-Fresnel thermal emission solver of libsmrt_dort.so (include/smrt_dort.h: smrt_multifresnel_*): its two kernels --
// one lane per (pair, layer slot) for the layer electromagnetics, one lane per (pair, sensor angle) for the chain of layer
// matrices; arithmetic in multifresnel_kernel.hpp -- and the host side: buffers on the DORT context, upload / launch / sync /
// download and the one-shot call.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <string>

#include "dort_ctx.hpp"
#include "multifresnel_kernel.hpp"
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

struct MultiFresnelState {
    DevBuf nl, thick, fv, temp, p1, p2, freq, mu, lw, kind, sub1, sub2, subT, pairmap;
    DevBuf stage, out, status, used, tau, layer;
    MfBatch dev{};
    bool uploaded = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timed = false;
};

namespace smrt_launch {
void multifresnel_release(smrt_dort_ctx* ctx) {
    MultiFresnelState* st = ctx->multifresnel;
    if (!st) return;
    DevBuf* bufs[] = {&st->nl, &st->thick, &st->fv, &st->temp, &st->p1, &st->p2, &st->freq, &st->mu, &st->lw, &st->kind, &st->sub1,
                      &st->sub2, &st->subT, &st->pairmap, &st->stage, &st->out, &st->status, &st->used, &st->tau, &st->layer};
    for (DevBuf* b : bufs) b->release();
    for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
    delete st;
    ctx->multifresnel = nullptr;
}
}  // namespace smrt_launch

static int mf_upload(smrt_dort_ctx* ctx, DevBuf& buf, const void* src, size_t bytes) {
    HIPCHK(buf.reserve(bytes));
    HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

static const char* mf_validate(const smrt_batch* b, const double* mu, double prune, int32_t prune_none) {
    if (!b) return "null batch";
    if (b->n_snowpacks <= 0 || b->n_frequencies <= 0 || b->n_layers_max <= 0) return "empty batch";
    if (b->n_theta <= 0 || !mu) return "the sensor cosines are missing";
    if (b->mode != SMRT_MODE_PASSIVE) return "the multi-Fresnel thermal emission solver needs a passive sensor";
    if (b->atm_tb_down || b->atm_tb_up || b->atm_transmittance) return "the multi-Fresnel thermal emission solver can not handle atmosphere";
    if (b->host_interface_slot) return "the multi-Fresnel thermal emission solver takes Flat interfaces only";
    if (b->host_layer || b->host_phase || b->host_iba_coeff) return "the multi-Fresnel thermal emission solver needs emmodels with a device implementation";
    if (b->process_coherent_layers) return "process_coherent_layers is not available in the multi-Fresnel thermal emission solver";
    if (b->emmodel < SMRT_EM_IBA || b->emmodel > SMRT_EM_RAYLEIGH_HOST) return "unknown emmodel";
    if (b->microstructure < SMRT_MS_EXPONENTIAL || b->microstructure > SMRT_MS_TEUBNER_STREY) return "unknown microstructure";
    if (!b->n_layers || !b->thickness || !b->frac_volume || !b->temperature || !b->micro_p1 || !b->frequency) return "null input array";
    if ((b->microstructure == SMRT_MS_STICKY_HARD_SPHERES || b->layer_kind) && !b->micro_p2) return "stickiness array missing";
    auto on_device = [](int em) { return em == SMRT_EM_IBA || em == SMRT_EM_DMRT_QCA_SHORTRANGE || em == SMRT_EM_DMRT_QCACP_SHORTRANGE ||
                                         em == SMRT_EM_NONSCATTERING || em == SMRT_EM_IBA_INVERTED; };
    auto dmrt = [](int em) { return em == SMRT_EM_DMRT_QCA_SHORTRANGE || em == SMRT_EM_DMRT_QCACP_SHORTRANGE; };
    if (!b->layer_kind) {
        if (!on_device(b->emmodel)) return "the multi-Fresnel thermal emission solver needs emmodels with a device implementation";
        if (dmrt(b->emmodel) && b->microstructure != SMRT_MS_STICKY_HARD_SPHERES)
            return "the dmrt short-range emmodels are only compatible with sticky_hard_spheres";
    }
    for (int s = 0; s < b->n_snowpacks; ++s) {
        if (b->n_layers[s] < 1 || b->n_layers[s] > b->n_layers_max) return "n_layers out of range";
        for (int l = 0; b->layer_kind && l < b->n_layers[s]; ++l) {
            const int k = b->layer_kind[(long long)s * b->n_layers_max + l], em = k & 15, ms = k >> 4;
            if (ms < SMRT_MS_EXPONENTIAL || ms > SMRT_MS_TEUBNER_STREY) return "invalid layer_kind entry";
            if (!on_device(em)) return "the multi-Fresnel thermal emission solver needs emmodels with a device implementation";
            if (dmrt(em) && ms != SMRT_MS_STICKY_HARD_SPHERES) return "the dmrt short-range emmodels are only compatible with sticky_hard_spheres";
        }
    }
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE && b->substrate_kind != SMRT_SUBSTRATE_FLAT)
        return "the multi-Fresnel thermal emission solver takes no substrate or a Flat one";
    if (b->substrate_kind == SMRT_SUBSTRATE_FLAT && (!b->substrate_p1 || !b->substrate_p2 || !b->substrate_temperature))
        return "substrate arrays missing";
    if (!prune_none && std::isnan(prune)) return "prune_deep_snowpack is not a number";
    return nullptr;
}

extern "C" {

int32_t smrt_multifresnel_out_stride(const smrt_batch* b) { return b ? 2 * b->n_theta : -1; }

int32_t smrt_multifresnel_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const double* mu, double prune_deep_snowpack,
                                       int32_t prune_none, const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = mf_validate(b, mu, prune_deep_snowpack, prune_none);
    if (why) { ctx->err = why; return -1; }
    const int64_t all = (int64_t)b->n_snowpacks * b->n_frequencies;
    if (!pairs) n_pairs = all;
    else {
        if (n_pairs <= 0) { ctx->err = "empty pair list"; return -1; }
        for (int64_t i = 0; i < n_pairs; ++i)
            if (pairs[i] < 0 || pairs[i] >= all) { ctx->err = "pair index out of bounds"; return -1; }
    }
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->multifresnel) {
        ctx->multifresnel = new MultiFresnelState();
        for (hipEvent_t& e : ctx->multifresnel->ev) HIPCHK(hipEventCreate(&e));
    }
    MultiFresnelState* st = ctx->multifresnel;
    st->uploaded = false;
    const size_t S = b->n_snowpacks, L = b->n_layers_max, F = b->n_frequencies, T = b->n_theta, N = (size_t)n_pairs;
    const size_t SL = S * L * sizeof(double), FS = F * S;
    MfBatch d{};
    d.S = (int)S; d.Lmax = (int)L; d.F = (int)F; d.n_theta = (int)T;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.sub_kind = b->substrate_kind;
    d.prune = prune_none ? INFINITY : prune_deep_snowpack;
    d.steepest = 0;
    for (size_t t = 1; t < T; ++t) if (mu[t] > mu[d.steepest]) d.steepest = (int)t;
    d.n_pairs = n_pairs;
#define MF_UP(buf, src, bytes, field) do { if (mf_upload(ctx, st->buf, src, bytes)) return -1; d.field = (decltype(d.field))st->buf.p; } while (0)
    MF_UP(nl, b->n_layers, S * sizeof(int32_t), n_layers);
    MF_UP(thick, b->thickness, SL, thickness);
    MF_UP(fv, b->frac_volume, SL, frac_volume);
    MF_UP(temp, b->temperature, SL, temperature);
    MF_UP(p1, b->micro_p1, SL, p1);
    if (b->micro_p2) MF_UP(p2, b->micro_p2, SL, p2);
    MF_UP(freq, b->frequency, F * sizeof(double), frequency);
    MF_UP(mu, mu, T * sizeof(double), mu);
    if (b->liquid_water) MF_UP(lw, b->liquid_water, SL, liquid_water);
    if (b->layer_kind) MF_UP(kind, b->layer_kind, S * L * sizeof(int32_t), layer_kind);
    if (b->substrate_kind == SMRT_SUBSTRATE_FLAT) {
        MF_UP(sub1, b->substrate_p1, FS * sizeof(double), sub_p1);
        MF_UP(sub2, b->substrate_p2, FS * sizeof(double), sub_p2);
        MF_UP(subT, b->substrate_temperature, S * sizeof(double), sub_T);
    }
    if (pairs) MF_UP(pairmap, pairs, N * sizeof(int64_t), pair_map);
#undef MF_UP
    HIPCHK(st->stage.reserve((size_t)MF_ROWS * (L + 1) * N * sizeof(double)));
    HIPCHK(st->out.reserve(N * 2 * T * sizeof(double)));
    HIPCHK(st->status.reserve(N * T * sizeof(int32_t)));
    HIPCHK(st->used.reserve(N * sizeof(int32_t)));
    HIPCHK(st->tau.reserve(N * sizeof(double)));
    HIPCHK(st->layer.reserve(N * L * 5 * sizeof(double)));
    d.stage = (double*)st->stage.p; d.out = (double*)st->out.p; d.status = (int*)st->status.p;
    d.layers_used = (int*)st->used.p; d.tau_snowpack = (double*)st->tau.p; d.layer_out = (double*)st->layer.p;
    // the copies above read the caller's (pageable) arrays: wait for them, the arrays may go away or change after this call
    HIPCHK(hipStreamSynchronize(ctx->stream));
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
    HIPCHK(hipEventRecord(st->ev[0], ctx->stream));
    hipLaunchKernelGGL(multifresnel_layers_kernel, dim3((unsigned)((items_a + kMfThreads - 1) / kMfThreads)), dim3(kMfThreads), 0,
                       ctx->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[1], ctx->stream));
    hipLaunchKernelGGL(multifresnel_chain_kernel, dim3((unsigned)((items_b + kMfThreads - 1) / kMfThreads)), dim3(kMfThreads), 0,
                       ctx->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[2], ctx->stream));
    st->timed = true;
    return 0;
}

int32_t smrt_multifresnel_sync(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_multifresnel_kernel_ms(smrt_dort_ctx* ctx, double* ms2) {
    if (!ctx || !ms2) return -1;
    MultiFresnelState* st = ctx->multifresnel;
    if (!st || !st->timed) { ctx->err = "no multi-Fresnel launch to time"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(st->ev[2]));
    float a = 0.f, c = 0.f;
    HIPCHK(hipEventElapsedTime(&a, st->ev[0], st->ev[1]));
    HIPCHK(hipEventElapsedTime(&c, st->ev[1], st->ev[2]));
    ms2[0] = a; ms2[1] = c;
    return 0;
}

int32_t smrt_multifresnel_download(smrt_dort_ctx* ctx, double* out, int32_t* status, int32_t* layers_used, double* tau_snowpack,
                                   double* layer_out) {
    if (!ctx) return -1;
    MultiFresnelState* st = ctx->multifresnel;
    if (!st || !st->uploaded) { ctx->err = "no multi-Fresnel batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const MfBatch& d = st->dev;
    const size_t N = (size_t)d.n_pairs, L = d.Lmax, T = d.n_theta;
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, N * 2 * T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, N * T * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (layers_used) HIPCHK(hipMemcpyAsync(layers_used, d.layers_used, N * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (tau_snowpack) HIPCHK(hipMemcpyAsync(tau_snowpack, d.tau_snowpack, N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.layer_out, N * L * 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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
