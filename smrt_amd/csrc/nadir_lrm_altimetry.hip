// The nadir LRM altimetry solver of libsmrt_dort.so (include/smrt_dort.h: smrt_lrm_*): its three kernels -- one lane per
// (pair, layer) for the layer scalars, one workgroup per pair for the vertical scattering distribution, one workgroup per
// (pair, output row) for the waveform; arithmetic in nadir_lrm_altimetry_kernel.hpp -- and the host side: buffers on the DORT
// context, upload / launch / sync / download and the one-shot call.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <string>

#include "nadir_lrm_altimetry_kernel.hpp"
#include "solver_host.hpp"
#include "solver_refusals.hpp"

using namespace smrt;

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

struct LrmState : solver_host::InputState {
    DevBuf &hostlayer = buf(), &hostcoeff = buf(), &tinc = buf(), &sigma = buf(), &slope = buf(), &itf = buf();
    DevBuf &stage = buf(), &bs = buf(), &prefix = buf(), &vsd = buf(), &out = buf(), &zgate = buf(), &status = buf(), &layer = buf();
    LrmBatch dev{};
    size_t lds_vertical = 0, lds_waveform = 0;
    bool uploaded = false;
    bool timed = false;   // events 0 .. 3 around the three kernels of the last launch
};

namespace smrt_launch {
void lrm_release(smrt_dort_ctx* ctx) { solver_host::release(ctx->lrm); }
}  // namespace smrt_launch

static int lrm_rows(const smrt_lrm_params* p) { return p->n_mu > 1 ? 2 * p->n_mu + 1 : p->return_contributions ? 3 : 1; }
static int lrm_out_rows(const smrt_lrm_params* p) { return p->return_contributions ? 3 : p->skip_pfs_convolution ? lrm_rows(p) : 1; }

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
    return solver_host::copy_table(desc, out, capacity);
}

int32_t smrt_lrm_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const smrt_lrm_params* p, const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = solver_refusals::nadir_lrm_altimetry(b, p);
    if (why) { ctx->err = why; return -1; }
    if (solver_host::check_pairs(ctx, pairs, &n_pairs, (int64_t)b->n_snowpacks * b->n_frequencies)) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->lrm) ctx->lrm = new LrmState();
    LrmState* st = ctx->lrm;
    st->uploaded = false;
    const size_t S = b->n_snowpacks, L = b->n_layers_max, F = b->n_frequencies, NP = (size_t)n_pairs;
    const size_t FSL = F * S * L;
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
    using solver_host::upload;
    if (solver_host::upload_batch(ctx, st, b, pairs, fo)) return -1;   // (fo.sub_kind is none: the substrate is not read)
    if (b->host_layer && upload(ctx, st->hostlayer, b->host_layer, FSL * 4 * sizeof(double), fo.host_layer)) return -1;
    if (b->host_iba_coeff && upload(ctx, st->hostcoeff, b->host_iba_coeff, FSL * sizeof(double), fo.host_coeff)) return -1;
    if (p->n_mu > 1 && upload(ctx, st->tinc, p->t_inc, p->n_mu * sizeof(double), d.t_inc)) return -1;
    if (p->sigma_surface && upload(ctx, st->sigma, p->sigma_surface, S * sizeof(double), d.sigma_surface)) return -1;
    if (p->surface_slope && upload(ctx, st->slope, p->surface_slope, S * sizeof(double), d.surface_slope)) return -1;
    if (p->interface_values && upload(ctx, st->itf, p->interface_values, F * S * (L + 1) * (1 + p->n_mu) * sizeof(double), d.itf)) return -1;
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
    if (solver_host::uploads_done(ctx)) return -1;
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
    st->rewind();
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(lrm_layers_kernel, dim3((unsigned)((items + kLrmThreads - 1) / kLrmThreads)), dim3(kLrmThreads), 0, ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(lrm_vertical_kernel, dim3((unsigned)d.fo.n_pairs), dim3(kLrmThreads), st->lds_vertical, ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(lrm_waveform_kernel, dim3((unsigned)(d.fo.n_pairs * d.out_rows)), dim3(kLrmThreads), st->lds_waveform, ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
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

int32_t smrt_lrm_sync(smrt_dort_ctx* ctx) { return solver_host::sync(ctx); }

int32_t smrt_lrm_kernel_ms(smrt_dort_ctx* ctx, double* ms3) {
    if (!ctx || !ms3) return -1;
    LrmState* st = ctx->lrm;
    if (!st || !st->timed) { ctx->err = "no altimetry launch to time"; return -1; }
    if (solver_host::wait_recorded(ctx, st)) return -1;
    for (int k = 0; k < 3; ++k) {
        ms3[k] = 0.0;
        if (solver_host::add_elapsed(ctx, st, k, k + 1, &ms3[k])) return -1;
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
