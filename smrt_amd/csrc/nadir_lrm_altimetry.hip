// The nadir LRM altimetry solver of libsmrt_dort.so (include/smrt_dort.h: smrt_lrm_*): its three kernels -- one lane per
// (pair, layer) for the layer scalars, one workgroup per pair for the vertical scattering distribution, one workgroup per
// (pair, output row) for the waveform; arithmetic in nadir_lrm_altimetry_kernel.hpp -- and the host side: buffers on the DORT
// context, upload / launch / sync / download and the one-shot call.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <string>

#include "dort_ctx.hpp"
#include "nadir_lrm_altimetry_kernel.hpp"
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

constexpr size_t kLrmLdsLimit = 160 * 1024 - 64;   // dynamic LDS of a workgroup: the 160 KB of a CU less the kernels' static bytes

__global__ void __launch_bounds__(kLrmThreads) lrm_layers_kernel(LrmBatch b) {
    const long long idx = (long long)blockIdx.x * kLrmThreads + threadIdx.x;
    if (idx >= b.fo.n_pairs * b.fo.Lmax) return;
    lrm_layer_item(b, idx % b.fo.n_pairs, (int)(idx / b.fo.n_pairs));   // pairs fastest: the staging rows are written with unit stride
}

__global__ void __launch_bounds__(kLrmThreads) lrm_vertical_kernel(LrmBatch b) {
    extern __shared__ double lrm_vertical_lds[];
    __shared__ double wsum[kLrmThreads / 64];
    LrmLane ln;
    ln.tid = threadIdx.x; ln.nt = kLrmThreads; ln.wsum = wsum;
    lrm_vertical_pair(b, blockIdx.x, ln, (unsigned char*)lrm_vertical_lds);
}

__global__ void __launch_bounds__(kLrmThreads) lrm_waveform_kernel(LrmBatch b) {
    extern __shared__ double lrm_waveform_lds[];
    LrmLane ln;
    ln.tid = threadIdx.x; ln.nt = kLrmThreads; ln.wsum = nullptr;
    lrm_waveform_item(b, blockIdx.x / b.out_rows, (int)(blockIdx.x % b.out_rows), ln, (unsigned char*)lrm_waveform_lds);
}

struct LrmState {
    DevBuf nl, thick, fv, temp, p1, p2, freq, lw, kind, hostlayer, hostcoeff, pairmap, tinc, sigma, slope, itf;
    DevBuf stage, bs, prefix, vsd, out, zgate, status, layer;
    LrmBatch dev{};
    size_t lds_vertical = 0, lds_waveform = 0;
    bool uploaded = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed = false;
};

namespace smrt_launch {
void lrm_release(smrt_dort_ctx* ctx) {
    LrmState* st = ctx->lrm;
    if (!st) return;
    DevBuf* bufs[] = {&st->nl, &st->thick, &st->fv, &st->temp, &st->p1, &st->p2, &st->freq, &st->lw, &st->kind, &st->hostlayer,
                      &st->hostcoeff, &st->pairmap, &st->tinc, &st->sigma, &st->slope, &st->itf, &st->stage, &st->bs, &st->prefix,
                      &st->vsd, &st->out, &st->zgate, &st->status, &st->layer};
    for (DevBuf* b : bufs) b->release();
    for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
    delete st;
    ctx->lrm = nullptr;
}
}  // namespace smrt_launch

static int lrm_upload(smrt_dort_ctx* ctx, DevBuf& buf, const void* src, size_t bytes) {
    HIPCHK(buf.reserve(bytes));
    HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

static int lrm_rows(const smrt_lrm_params* p) { return p->n_mu > 1 ? 2 * p->n_mu + 1 : p->return_contributions ? 3 : 1; }
static int lrm_out_rows(const smrt_lrm_params* p) { return p->return_contributions ? 3 : p->skip_pfs_convolution ? lrm_rows(p) : 1; }

static const char* lrm_validate(const smrt_batch* b, const smrt_lrm_params* p) {
    if (!b || !p) return "null batch or parameters";
    if (b->n_snowpacks <= 0 || b->n_frequencies <= 0 || b->n_layers_max <= 0) return "empty batch";
    if (b->atm_tb_down || b->atm_tb_up || b->atm_transmittance) return "the nadir LRM altimetry solver can not handle atmosphere";
    if (b->host_phase) return "the nadir LRM altimetry solver has no route for phase matrices evaluated on the host";
    if (b->process_coherent_layers) return "process_coherent_layers is not available in the nadir LRM altimetry solver";
    if (b->emmodel < SMRT_EM_IBA || b->emmodel > SMRT_EM_RAYLEIGH_HOST) return "unknown emmodel";
    if (b->microstructure < SMRT_MS_EXPONENTIAL || b->microstructure > SMRT_MS_TEUBNER_STREY) return "unknown microstructure";
    if (!b->n_layers || !b->thickness || !b->frac_volume || !b->temperature || !b->micro_p1 || !b->frequency) return "null input array";
    if ((b->microstructure == SMRT_MS_STICKY_HARD_SPHERES || b->layer_kind) && !b->micro_p2) return "stickiness array missing";
    for (int s = 0; s < b->n_snowpacks; ++s) {
        if (b->n_layers[s] < 1 || b->n_layers[s] > b->n_layers_max) return "n_layers out of range";
        for (int l = 0; b->layer_kind && l < b->n_layers[s]; ++l) {
            const int ms = b->layer_kind[(long long)s * b->n_layers_max + l] >> 4;
            if (ms < SMRT_MS_EXPONENTIAL || ms > SMRT_MS_TEUBNER_STREY) return "invalid layer_kind entry";
        }
    }
    if (p->ngate < 1 || p->oversampling < 1) return "ngate and oversampling_time must be positive";
    if ((long long)p->ngate * p->oversampling > (1 << 20)) return "ngate x oversampling_time is too large";
    if (p->n_mu < 1 || (p->n_mu > 1 && !p->t_inc)) return "the times of the incidence samples are missing";
    if (p->n_mu > 1 && p->skip_pfs_convolution) return "skip_pfs_convolution needs theta_inc_sampling = 1";
    if (!(p->altitude > 0.0) || !(p->pulse_bandwidth > 0.0) || !(p->gamma > 0.0) || !(p->pulse_sigma > 0.0)) return "invalid sensor parameters";
    if (p->n_mu == 1 && !p->skip_pfs_convolution && (p->shift < 1 || p->shift >= p->ngate * p->oversampling))
        return "the nominal gate must lie inside the gate window, after its first sub-gate";
    if (p->n_mu > 1 && p->sigma_surface) return "sigma_surface needs theta_inc_sampling = 1";
    const size_t a = lrm_vertical_lds_bytes(p->ngate * p->oversampling, b->n_layers_max);
    const size_t c = lrm_waveform_lds_bytes(p->ngate * p->oversampling, p->n_mu);
    if (a > kLrmLdsLimit || c > kLrmLdsLimit) return "ngate x oversampling_time (and the layers) do not fit the local data share";
    return nullptr;
}

extern "C" {

int32_t smrt_lrm_out_stride(const smrt_lrm_params* p) {
    if (!p || p->ngate < 1 || p->oversampling < 1 || p->n_mu < 1) return -1;
    return lrm_out_rows(p) * (p->return_oversampled ? p->ngate * p->oversampling : p->ngate);
}

int32_t smrt_lrm_abi(int32_t* out, int32_t capacity) {
#define SMRT_OFF(f) (int32_t)offsetof(smrt_lrm_params, f)
    const int32_t desc[] = {(int32_t)sizeof(smrt_lrm_params), SMRT_OFF(altitude), SMRT_OFF(pulse_bandwidth), SMRT_OFF(antenna_gain),
                            SMRT_OFF(gamma), SMRT_OFF(off_nadir_angle), SMRT_OFF(nominal_gate), SMRT_OFF(pulse_sigma), SMRT_OFF(ngate),
                            SMRT_OFF(oversampling), SMRT_OFF(n_mu), SMRT_OFF(shift), SMRT_OFF(return_contributions),
                            SMRT_OFF(return_oversampled), SMRT_OFF(skip_pfs_convolution), SMRT_OFF(reserved), SMRT_OFF(t_inc),
                            SMRT_OFF(sigma_surface), SMRT_OFF(surface_slope), SMRT_OFF(interface_values)};
#undef SMRT_OFF
    const int32_t n = (int32_t)(sizeof(desc) / sizeof(desc[0]));
    for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = desc[i];
    return n;
}

int32_t smrt_lrm_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const smrt_lrm_params* p, const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = lrm_validate(b, p);
    if (why) { ctx->err = why; return -1; }
    const int64_t all = (int64_t)b->n_snowpacks * b->n_frequencies;
    if (!pairs) n_pairs = all;
    else {
        if (n_pairs <= 0) { ctx->err = "empty pair list"; return -1; }
        for (int64_t i = 0; i < n_pairs; ++i)
            if (pairs[i] < 0 || pairs[i] >= all) { ctx->err = "pair index out of bounds"; return -1; }
    }
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->lrm) {
        ctx->lrm = new LrmState();
        for (hipEvent_t& e : ctx->lrm->ev) HIPCHK(hipEventCreate(&e));
    }
    LrmState* st = ctx->lrm;
    st->uploaded = false;
    const size_t S = b->n_snowpacks, L = b->n_layers_max, F = b->n_frequencies, NP = (size_t)n_pairs;
    const size_t SL = S * L * sizeof(double), FSL = F * S * L;
    LrmBatch d{};
    FoBatch& fo = d.fo;
    fo.S = (int)S; fo.Lmax = (int)L; fo.F = (int)F; fo.n_theta = 1;
    fo.emmodel = b->emmodel; fo.micro = b->microstructure; fo.sub_kind = 0; fo.n_slots = 0;
    fo.n_pairs = n_pairs;
    d.ngate = p->ngate; d.os = p->oversampling; d.n_mu = p->n_mu; d.shift = p->shift;
    d.contributions = p->return_contributions ? 1 : 0; d.oversampled = p->return_oversampled ? 1 : 0;
    d.skip_pfs = p->skip_pfs_convolution ? 1 : 0;
    d.N = p->ngate * p->oversampling;
    d.rows = lrm_rows(p); d.out_rows = lrm_out_rows(p); d.n_out = d.oversampled ? d.N : d.ngate;
    d.altitude = p->altitude; d.bandwidth = p->pulse_bandwidth; d.gain = p->antenna_gain; d.gamma = p->gamma;
    d.off_nadir = p->off_nadir_angle; d.nominal_gate = p->nominal_gate; d.pulse_sigma = p->pulse_sigma;
#define LRM_UP(buf, src, bytes, field) do { if (lrm_upload(ctx, st->buf, src, bytes)) return -1; field = (decltype(field))st->buf.p; } while (0)
    LRM_UP(nl, b->n_layers, S * sizeof(int32_t), fo.n_layers);
    LRM_UP(thick, b->thickness, SL, fo.thickness);
    LRM_UP(fv, b->frac_volume, SL, fo.frac_volume);
    LRM_UP(temp, b->temperature, SL, fo.temperature);
    LRM_UP(p1, b->micro_p1, SL, fo.p1);
    if (b->micro_p2) LRM_UP(p2, b->micro_p2, SL, fo.p2);
    LRM_UP(freq, b->frequency, F * sizeof(double), fo.frequency);
    if (b->liquid_water) LRM_UP(lw, b->liquid_water, SL, fo.liquid_water);
    if (b->layer_kind) LRM_UP(kind, b->layer_kind, S * L * sizeof(int32_t), fo.layer_kind);
    if (b->host_layer) LRM_UP(hostlayer, b->host_layer, FSL * 4 * sizeof(double), fo.host_layer);
    if (b->host_iba_coeff) LRM_UP(hostcoeff, b->host_iba_coeff, FSL * sizeof(double), fo.host_coeff);
    if (pairs) LRM_UP(pairmap, pairs, NP * sizeof(int64_t), fo.pair_map);
    if (p->n_mu > 1) LRM_UP(tinc, p->t_inc, p->n_mu * sizeof(double), d.t_inc);
    if (p->sigma_surface) LRM_UP(sigma, p->sigma_surface, S * sizeof(double), d.sigma_surface);
    if (p->surface_slope) LRM_UP(slope, p->surface_slope, S * sizeof(double), d.surface_slope);
    if (p->interface_values) LRM_UP(itf, p->interface_values, F * S * (L + 1) * (1 + p->n_mu) * sizeof(double), d.itf);
#undef LRM_UP
    HIPCHK(st->stage.reserve((size_t)FO_ROWS * L * NP * sizeof(double)));
    HIPCHK(st->bs.reserve(L * NP * sizeof(double)));
    HIPCHK(st->prefix.reserve(NP * LRM_PREFIX_ROWS * (L + 1) * sizeof(double)));
    HIPCHK(st->vsd.reserve(NP * d.rows * d.N * sizeof(double)));
    HIPCHK(st->out.reserve(NP * d.out_rows * d.n_out * sizeof(double)));
    HIPCHK(st->zgate.reserve(NP * d.n_out * sizeof(double)));
    HIPCHK(st->status.reserve(NP * sizeof(int32_t)));
    HIPCHK(st->layer.reserve(NP * L * 5 * sizeof(double)));
    fo.stage = (double*)st->stage.p; fo.layer_out = (double*)st->layer.p;
    d.bs = (double*)st->bs.p; d.prefix = (double*)st->prefix.p; d.vsd = (double*)st->vsd.p; d.out = (double*)st->out.p;
    d.z_gate = (double*)st->zgate.p; d.status = (int*)st->status.p;
    st->lds_vertical = lrm_vertical_lds_bytes(d.N, (int)L);
    st->lds_waveform = lrm_waveform_lds_bytes(d.N, d.n_mu);
    // the copies above read the caller's (pageable) arrays: wait for them, the arrays may go away or change after this call
    HIPCHK(hipStreamSynchronize(ctx->stream));
    st->dev = d;
    st->uploaded = true;
    st->timed = false;
    return 0;
}

int32_t smrt_lrm_launch(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    LrmState* st = ctx->lrm;
    if (!st || !st->uploaded) { ctx->err = "no altimetry batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const LrmBatch& d = st->dev;
    const long long items = d.fo.n_pairs * d.fo.Lmax;
    // (a per-function setting shared by every context of the process: set for THIS batch at every launch)
    HIPCHK(hipFuncSetAttribute((const void*)lrm_vertical_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st->lds_vertical));
    HIPCHK(hipFuncSetAttribute((const void*)lrm_waveform_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st->lds_waveform));
    HIPCHK(hipEventRecord(st->ev[0], ctx->stream));
    hipLaunchKernelGGL(lrm_layers_kernel, dim3((unsigned)((items + kLrmThreads - 1) / kLrmThreads)), dim3(kLrmThreads), 0, ctx->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[1], ctx->stream));
    hipLaunchKernelGGL(lrm_vertical_kernel, dim3((unsigned)d.fo.n_pairs), dim3(kLrmThreads), st->lds_vertical, ctx->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[2], ctx->stream));
    hipLaunchKernelGGL(lrm_waveform_kernel, dim3((unsigned)(d.fo.n_pairs * d.out_rows)), dim3(kLrmThreads), st->lds_waveform, ctx->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[3], ctx->stream));
    st->timed = true;
    return 0;
}

int32_t smrt_lrm_layers(smrt_dort_ctx* ctx, double* layer_out) {
    if (!ctx || !layer_out) return -1;
    LrmState* st = ctx->lrm;
    if (!st || !st->uploaded) { ctx->err = "no altimetry batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const LrmBatch& d = st->dev;
    const long long items = d.fo.n_pairs * d.fo.Lmax;
    hipLaunchKernelGGL(lrm_layers_kernel, dim3((unsigned)((items + kLrmThreads - 1) / kLrmThreads)), dim3(kLrmThreads), 0, ctx->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(layer_out, d.fo.layer_out, (size_t)items * 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_lrm_sync(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_lrm_kernel_ms(smrt_dort_ctx* ctx, double* ms3) {
    if (!ctx || !ms3) return -1;
    LrmState* st = ctx->lrm;
    if (!st || !st->timed) { ctx->err = "no altimetry launch to time"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(st->ev[3]));
    for (int k = 0; k < 3; ++k) {
        float a = 0.f;
        HIPCHK(hipEventElapsedTime(&a, st->ev[k], st->ev[k + 1]));
        ms3[k] = a;
    }
    return 0;
}

int32_t smrt_lrm_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* z_gate, double* layer_out, double* vertical) {
    if (!ctx) return -1;
    LrmState* st = ctx->lrm;
    if (!st || !st->uploaded) { ctx->err = "no altimetry batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const LrmBatch& d = st->dev;
    const size_t NP = (size_t)d.fo.n_pairs, L = d.fo.Lmax;
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, NP * d.out_rows * d.n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, NP * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (z_gate) HIPCHK(hipMemcpyAsync(z_gate, d.z_gate, NP * d.n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.fo.layer_out, NP * L * 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (vertical) HIPCHK(hipMemcpyAsync(vertical, d.vsd, NP * d.rows * d.N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_lrm_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_lrm_params* params, const int64_t* pairs,
                           int64_t n_pairs, double* out, int32_t* status, double* z_gate, double* layer_out, double* vertical) {
    if (smrt_lrm_upload_pairs(ctx, batch, params, pairs, n_pairs)) return -1;
    if (smrt_lrm_launch(ctx)) return -1;
    return smrt_lrm_download(ctx, out, status, z_gate, layer_out, vertical);
}

}  // extern "C"
