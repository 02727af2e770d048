// The nadir LRM altimetry solver of libsmrt_dort.so (include/smrt_dort.h: smrt_lrm_*): its three kernels -- one lane per
// (pair, layer) for the layer scalars, one workgroup per pair for the vertical scattering distribution, one workgroup per
// (pair, output row) for the waveform; arithmetic in nadir_lrm_altimetry_kernel.hpp -- and the host side: buffers on the DORT
// context, upload / launch / sync / download and the one-shot call.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <string>

#include "solver_describe.hpp"
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

extern "C" {

int32_t smrt_lrm_out_stride(const smrt_lrm_params* p) {
    if (!p || p->ngate < 1 || p->oversampling < 1 || p->n_mu < 1) return -1;
    return solver_describe::lrm_out_rows(p) * (p->return_oversampled ? p->ngate * p->oversampling : p->ngate);
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
    LrmBatch d = solver_describe::nadir_lrm_altimetry(b, p, n_pairs);
    FoBatch& fo = d.fo;
    const solver_describe::LrmExtents n = solver_describe::extents(d);
    const solver_describe::FoExtents nf = solver_describe::extents(fo);
    using solver_host::upload;
    if (solver_host::upload_batch(ctx, st, b, pairs, fo)) return -1;   // (fo.sub_kind is none: the substrate is not read)
    if (b->host_layer && upload(ctx, st->hostlayer, b->host_layer, nf.host_layer * sizeof(double), fo.host_layer)) return -1;
    if (b->host_iba_coeff && upload(ctx, st->hostcoeff, b->host_iba_coeff, nf.host_coeff * sizeof(double), fo.host_coeff)) return -1;
    if (p->n_mu > 1 && upload(ctx, st->tinc, p->t_inc, n.t_inc * sizeof(double), d.t_inc)) return -1;
    if (p->sigma_surface && upload(ctx, st->sigma, p->sigma_surface, n.per_snowpack * sizeof(double), d.sigma_surface)) return -1;
    if (p->surface_slope && upload(ctx, st->slope, p->surface_slope, n.per_snowpack * sizeof(double), d.surface_slope)) return -1;
    if (p->interface_values && upload(ctx, st->itf, p->interface_values, n.itf * sizeof(double), d.itf)) return -1;
    using solver_host::reserve;
    if (reserve(ctx, st->stage, n.stage, fo.stage) || reserve(ctx, st->bs, n.bs, d.bs) || reserve(ctx, st->prefix, n.prefix, d.prefix) ||
        reserve(ctx, st->vsd, n.vsd, d.vsd) || reserve(ctx, st->out, n.out, d.out) || reserve(ctx, st->zgate, n.z_gate, d.z_gate) ||
        reserve(ctx, st->status, n.status, d.status) || reserve(ctx, st->layer, n.layer_out, fo.layer_out))
        return -1;
    st->lds_vertical = n.lds_vertical;
    st->lds_waveform = n.lds_waveform;
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
    HIPCHK(hipMemcpyAsync(layer_out, d.fo.layer_out, solver_describe::extents(d).layer_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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
    const solver_describe::LrmExtents n = solver_describe::extents(d);
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, n.out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, n.status * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (z_gate) HIPCHK(hipMemcpyAsync(z_gate, d.z_gate, n.z_gate * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.fo.layer_out, n.layer_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (vertical) HIPCHK(hipMemcpyAsync(vertical, d.vsd, n.vsd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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
