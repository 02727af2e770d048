// The nadir SAR altimetry solver of libsmrt_dort.so (include/smrt_dort.h: smrt_sar_*): its four kernels -- one lane per
// (pair, layer) for the layer scalars, one workgroup per pair for the vertical distribution and the echo of the boundaries, one
// lane per sample of the f0 / f1 tables, one workgroup per (pair, coarse Doppler bin) for the map; arithmetic in
// nadir_sar_altimetry_kernel.hpp; with the model of Halimi et al. 2014 the table stage is three kernels (one workgroup per
// delay, per table, per table and Doppler column) and the map kernel its other instantiation -- and the host side: buffers on the DORT context, upload / launch / sync / download and the
// one-shot call.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <string>

#include "solver_describe.hpp"
#include "solver_host.hpp"
#include "solver_refusals.hpp"

using namespace smrt;

__global__ void __launch_bounds__(kSarThreads) sar_layers_kernel(SarBatch b) {
    const long long idx = (long long)blockIdx.x * kSarThreads + threadIdx.x;
    if (idx >= b.lrm.fo.n_pairs * b.lrm.fo.Lmax) return;
    lrm_layer_item(b.lrm, idx % b.lrm.fo.n_pairs, (int)(idx / b.lrm.fo.n_pairs));
}

__global__ void __launch_bounds__(kSarThreads) sar_vertical_kernel(SarBatch b) {
    extern __shared__ double sar_vertical_lds[];
    __shared__ double wsum[kSarThreads / 64];
    LrmLane ln;
    ln.tid = threadIdx.x; ln.nt = kSarThreads; ln.wsum = wsum;
    lrm_vertical_pair(b.lrm, blockIdx.x, ln, (unsigned char*)sar_vertical_lds);
    lrm_sync();
    sar_boundary_pair(b, blockIdx.x, threadIdx.x, kSarThreads);
}

__global__ void __launch_bounds__(kSarThreads) sar_tables_kernel(SarBatch b) {
    const long long idx = (long long)blockIdx.x * kSarThreads + threadIdx.x;
    if (idx >= (long long)b.n_tab * b.lrm.N * b.ND) return;
    sar_table_item(b, idx);
}

// The table stage of Halimi14: one workgroup per delay of the widened window, per table, per (table, Doppler column).
__global__ void __launch_bounds__(kSarThreads) sar_h14_doppler_kernel(SarBatch b) {
    extern __shared__ double sar_h14_doppler_lds[];
    sar_h14_doppler_row(b, (int)blockIdx.x, threadIdx.x, kSarThreads, (unsigned char*)sar_h14_doppler_lds);
}

__global__ void __launch_bounds__(kSarThreads) sar_h14_kernel_kernel(SarBatch b) {
    extern __shared__ double sar_h14_kernel_lds[];
    sar_h14_kernel_table(b, (int)blockIdx.x, threadIdx.x, kSarThreads, (unsigned char*)sar_h14_kernel_lds);
}

__global__ void __launch_bounds__(kSarThreads) sar_h14_delay_kernel(SarBatch b) {
    extern __shared__ double sar_h14_delay_lds[];
    sar_h14_delay_column(b, (int)(blockIdx.x / b.ND), (int)(blockIdx.x % b.ND), threadIdx.x, kSarThreads, (unsigned char*)sar_h14_delay_lds);
}

template <int MODEL>
__global__ void __launch_bounds__(kSarThreads) sar_combine_kernel(SarBatch b) {
    extern __shared__ double sar_combine_lds[];
    sar_combine_model<MODEL>(b, blockIdx.x / b.ndoppler, (int)(blockIdx.x % b.ndoppler), threadIdx.x, kSarThreads, (unsigned char*)sar_combine_lds);
}

struct SarState : solver_host::InputState {
    DevBuf &hostlayer = buf(), &hostcoeff = buf(), &tabsigma = buf(), &tabindex = buf(), &bv = buf(), &rowmap = buf();
    DevBuf &stage = buf(), &bs = buf(), &prefix = buf(), &vsd = buf(), &zgate = buf(), &status = buf(), &layer = buf();
    DevBuf &tables = buf(), &echo = buf(), &out = buf(), &h14doppler = buf(), &h14kernel = buf();
    SarBatch dev{};
    size_t lds_vertical = 0, lds_combine = 0, lds_h14_doppler = 0, lds_h14_kernel = 0, lds_h14_delay = 0;
    bool uploaded = false;
    bool timed = false;   // events 0 .. 4 around the four kernels of the last launch
};

namespace smrt_launch {
void sar_release(smrt_dort_ctx* ctx) { solver_host::release(ctx->sar); }
}  // namespace smrt_launch

extern "C" {

int32_t smrt_sar_out_stride(const smrt_sar_params* p) {
    if (!p || p->ngate < 1 || p->ndoppler < 1 || p->oversampling_time < 1 || p->oversampling_doppler < 1 || p->n_rows < 1) return -1;
    const long long n = (long long)p->n_rows * p->ngate * p->ndoppler * (p->return_oversampled ? p->oversampling_time * p->oversampling_doppler : 1);
    return n > 0x7fffffffLL ? -1 : (int32_t)n;
}

int32_t smrt_sar_abi(int32_t* out, int32_t capacity) {
#define SMRT_OFF(f) (int32_t)offsetof(smrt_sar_params, f)
    const int32_t desc[] = {(int32_t)sizeof(smrt_sar_params), SMRT_OFF(altitude), SMRT_OFF(pulse_bandwidth), SMRT_OFF(nominal_gate),
                            SMRT_OFF(pulse_repetition_frequency), SMRT_OFF(wavelength), SMRT_OFF(velocity), SMRT_OFF(alpha),
                            SMRT_OFF(pitch_angle), SMRT_OFF(roll_angle), SMRT_OFF(sigma_p), SMRT_OFF(theta_lim), SMRT_OFF(gamma_x),
                            SMRT_OFF(gamma_y), SMRT_OFF(l_gamma), SMRT_OFF(lz), SMRT_OFF(pu), SMRT_OFF(nu_coherent), SMRT_OFF(ngate),
                            SMRT_OFF(ndoppler), SMRT_OFF(oversampling_time), SMRT_OFF(oversampling_doppler), SMRT_OFF(return_oversampled),
                            SMRT_OFF(n_rows), SMRT_OFF(n_tables), SMRT_OFF(reserved), SMRT_OFF(table_sigma), SMRT_OFF(table_index),
                            SMRT_OFF(boundary_values), SMRT_OFF(row_map), SMRT_OFF(delay_doppler_model), SMRT_OFF(slant_range_correction),
                            SMRT_OFF(delay_window_widening), SMRT_OFF(reserved2), SMRT_OFF(h14_pu), SMRT_OFF(h14_gamma), SMRT_OFF(burst_duration)};
#undef SMRT_OFF
    return solver_host::copy_table(desc, out, capacity);
}

int32_t smrt_sar_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const smrt_sar_params* p, const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = solver_refusals::nadir_sar_altimetry(b, p);
    if (why) { ctx->err = why; return -1; }
    if (solver_host::check_pairs(ctx, pairs, &n_pairs, (int64_t)b->n_snowpacks)) return -1;
    const size_t NP = (size_t)n_pairs;
    const size_t stride = (size_t)smrt_sar_out_stride(p);
    if (NP * stride * sizeof(double) > solver_refusals::kSarOutputBudget) {
        ctx->err = "the maps of these pairs do not fit the output budget of the nadir SAR altimetry solver: launch fewer pairs at a time";
        return -1;
    }
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->sar) ctx->sar = new SarState();
    SarState* st = ctx->sar;
    st->uploaded = false;
    SarBatch d = solver_describe::nadir_sar_altimetry(b, p, n_pairs);
    LrmBatch& lb = d.lrm;
    FoBatch& fo = lb.fo;
    const solver_describe::SarExtents n = solver_describe::extents(d);
    const solver_describe::FoExtents nf = solver_describe::extents(fo);
    using solver_host::upload;
    if (solver_host::upload_batch(ctx, st, b, pairs, fo)) return -1;   // (fo.sub_kind is none: the substrate is not read)
    if (b->host_layer && upload(ctx, st->hostlayer, b->host_layer, nf.host_layer * sizeof(double), fo.host_layer)) return -1;
    if (b->host_iba_coeff && upload(ctx, st->hostcoeff, b->host_iba_coeff, nf.host_coeff * sizeof(double), fo.host_coeff)) return -1;
    if (upload(ctx, st->tabsigma, p->table_sigma, n.tab_sigma * sizeof(double), d.tab_sigma)) return -1;
    if (upload(ctx, st->tabindex, p->table_index, n.tab_index * sizeof(int32_t), d.tab_index)) return -1;
    if (upload(ctx, st->bv, p->boundary_values, n.boundary_values * sizeof(double), lb.itf)) return -1;
    if (upload(ctx, st->rowmap, p->row_map, n.row_map * sizeof(int32_t), d.row_map)) return -1;
    using solver_host::reserve;
    if (reserve(ctx, st->stage, n.lrm.stage, fo.stage) || reserve(ctx, st->bs, n.lrm.bs, lb.bs) || reserve(ctx, st->prefix, n.lrm.prefix, lb.prefix) ||
        reserve(ctx, st->vsd, n.lrm.vsd, lb.vsd) || reserve(ctx, st->zgate, n.lrm.z_gate, lb.z_gate) || reserve(ctx, st->status, n.lrm.status, lb.status) ||
        reserve(ctx, st->layer, n.lrm.layer_out, fo.layer_out) || reserve(ctx, st->tables, n.tables, d.tables))
        return -1;
    if (d.model == kSarHalimi14 && (reserve(ctx, st->h14doppler, n.h14_doppler, d.h14_doppler) || reserve(ctx, st->h14kernel, n.h14_kernel, d.h14_kernel)))
        return -1;
    if (reserve(ctx, st->echo, n.echo, d.echo) || reserve(ctx, st->out, n.out, d.out)) return -1;
    st->lds_vertical = n.lrm.lds_vertical;
    st->lds_combine = n.lds_combine;
    st->lds_h14_doppler = n.lds_h14_doppler;
    st->lds_h14_kernel = n.lds_h14_kernel;
    st->lds_h14_delay = n.lds_h14_delay;
    if (solver_host::uploads_done(ctx)) return -1;
    st->dev = d;
    st->uploaded = true;
    st->timed = false;
    return 0;
}

int32_t smrt_sar_launch(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    SarState* st = ctx->sar;
    if (!st || !st->uploaded) { ctx->err = "no SAR altimetry batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const SarBatch& d = st->dev;
    const long long items = d.lrm.fo.n_pairs * d.lrm.fo.Lmax, samples = (long long)d.n_tab * d.lrm.N * d.ND;
    // (a per-function setting shared by every context of the process: set for THIS batch at every launch)
    HIPCHK(hipFuncSetAttribute((const void*)sar_vertical_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st->lds_vertical));
    const bool h14 = d.model == kSarHalimi14;
    const void* combine = h14 ? (const void*)sar_combine_kernel<kSarHalimi14> : (const void*)sar_combine_kernel<kSarDinardo18>;
    HIPCHK(hipFuncSetAttribute(combine, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st->lds_combine));
    if (h14) {
        HIPCHK(hipFuncSetAttribute((const void*)sar_h14_doppler_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st->lds_h14_doppler));
        HIPCHK(hipFuncSetAttribute((const void*)sar_h14_kernel_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st->lds_h14_kernel));
        HIPCHK(hipFuncSetAttribute((const void*)sar_h14_delay_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st->lds_h14_delay));
    }
    st->rewind();
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(sar_layers_kernel, dim3((unsigned)((items + kSarThreads - 1) / kSarThreads)), dim3(kSarThreads), 0, ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(sar_vertical_kernel, dim3((unsigned)d.lrm.fo.n_pairs), dim3(kSarThreads), st->lds_vertical, ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    if (h14) {   // (the three kernels of the table stage between one pair of events: smrt_sar_kernel_ms sums them)
        hipLaunchKernelGGL(sar_h14_doppler_kernel, dim3((unsigned)d.N_wide), dim3(kSarThreads), st->lds_h14_doppler, ctx->stream, d);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(sar_h14_kernel_kernel, dim3((unsigned)d.n_tab), dim3(kSarThreads), st->lds_h14_kernel, ctx->stream, d);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(sar_h14_delay_kernel, dim3((unsigned)((long long)d.n_tab * d.ND)), dim3(kSarThreads), st->lds_h14_delay, ctx->stream, d);
    } else {
        hipLaunchKernelGGL(sar_tables_kernel, dim3((unsigned)((samples + kSarThreads - 1) / kSarThreads)), dim3(kSarThreads), 0, ctx->stream, d);
    }
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    if (h14)
        hipLaunchKernelGGL(sar_combine_kernel<kSarHalimi14>, dim3((unsigned)(d.lrm.fo.n_pairs * d.ndoppler)), dim3(kSarThreads), st->lds_combine, ctx->stream, d);
    else
        hipLaunchKernelGGL(sar_combine_kernel<kSarDinardo18>, dim3((unsigned)(d.lrm.fo.n_pairs * d.ndoppler)), dim3(kSarThreads), st->lds_combine, ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    st->timed = true;
    return 0;
}

int32_t smrt_sar_sync(smrt_dort_ctx* ctx) { return solver_host::sync(ctx); }

int32_t smrt_sar_kernel_ms(smrt_dort_ctx* ctx, double* ms4) {
    if (!ctx || !ms4) return -1;
    SarState* st = ctx->sar;
    if (!st || !st->timed) { ctx->err = "no SAR altimetry launch to time"; return -1; }
    if (solver_host::wait_recorded(ctx, st)) return -1;
    for (int k = 0; k < 4; ++k) {
        ms4[k] = 0.0;
        if (solver_host::add_elapsed(ctx, st, k, k + 1, &ms4[k])) return -1;
    }
    return 0;
}

int32_t smrt_sar_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* z_gate, double* layer_out, double* vertical, double* echo) {
    if (!ctx) return -1;
    SarState* st = ctx->sar;
    if (!st || !st->uploaded) { ctx->err = "no SAR altimetry batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const SarBatch& d = st->dev;
    const solver_describe::SarExtents n = solver_describe::extents(d);
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, n.out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.lrm.status, n.lrm.status * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (z_gate) HIPCHK(hipMemcpyAsync(z_gate, d.lrm.z_gate, n.lrm.z_gate * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.lrm.fo.layer_out, n.lrm.layer_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (vertical) HIPCHK(hipMemcpyAsync(vertical, d.lrm.vsd, n.lrm.vsd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (echo) HIPCHK(hipMemcpyAsync(echo, d.echo, n.echo * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_sar_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_sar_params* params, const int64_t* pairs,
                           int64_t n_pairs, double* out, int32_t* status, double* z_gate, double* layer_out, double* vertical, double* echo) {
    if (smrt_sar_upload_pairs(ctx, batch, params, pairs, n_pairs)) return -1;
    if (smrt_sar_launch(ctx)) return -1;
    return smrt_sar_download(ctx, out, status, z_gate, layer_out, vertical, echo);
}

}  // extern "C"
