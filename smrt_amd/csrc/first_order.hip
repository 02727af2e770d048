// The iterative first-order backscatter solver of libsmrt_dort.so (include/smrt_dort.h: smrt_first_order_*): its two
// kernels -- one lane per (pair, layer) for the layer electromagnetics, one lane per (pair, incidence angle) for the
// recursion; arithmetic in first_order_kernel.hpp -- and the host side: buffers on the DORT context, upload / launch /
// sync / download and the one-shot call.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>
#include <string>

#include "solver_describe.hpp"
#include "solver_host.hpp"
#include "solver_refusals.hpp"

using namespace smrt;

constexpr int kFoThreads = 256;

__global__ void __launch_bounds__(kFoThreads) first_order_layers_kernel(FoBatch b) {
    const long long idx = (long long)blockIdx.x * kFoThreads + threadIdx.x;
    if (idx >= b.n_pairs * b.Lmax) return;
    first_order_layer_item(b, idx % b.n_pairs, (int)(idx / b.n_pairs));   // pairs fastest: the staging rows are written with unit stride
}

__global__ void __launch_bounds__(kFoThreads) first_order_angles_kernel(FoBatch b) {
    const long long idx = (long long)blockIdx.x * kFoThreads + threadIdx.x;
    if (idx >= b.n_pairs * b.n_theta) return;
    first_order_angle_item(b, idx / b.n_theta, (int)(idx % b.n_theta));   // angles fastest: a wavefront reads 64 / n_theta consecutive staging entries and writes whole output rows
}

struct FirstOrderState : solver_host::InputState {
    DevBuf &theta = buf(), &hostlayer = buf(), &hostcoeff = buf(), &slot = buf(), &values = buf(), &phase = buf();
    DevBuf &stage = buf(), &out = buf(), &status = buf(), &layer = buf(), &lb = buf(), &diag = buf();
    FoBatch dev{};
    bool uploaded = false;
    bool timed = false;   // events 0, 1, 2 around the two kernels of the last launch
};

namespace smrt_launch {
void first_order_release(smrt_dort_ctx* ctx) { solver_host::release(ctx->first_order); }
FoBatch* first_order_resident(smrt_dort_ctx* ctx) {
    FirstOrderState* st = ctx->first_order;
    return st && st->uploaded ? &st->dev : nullptr;
}
}  // namespace smrt_launch

extern "C" {

int32_t smrt_first_order_out_stride(const smrt_batch* b) { return b ? 16 * b->n_theta : -1; }

int32_t smrt_first_order_abi(int32_t* out, int32_t capacity) {
#define SMRT_OFF(f) (int32_t)offsetof(smrt_first_order_extras, f)
    const int32_t desc[] = {(int32_t)sizeof(smrt_first_order_extras), SMRT_OFF(n_interface_slots), SMRT_OFF(reserved),
                            SMRT_OFF(host_interface_slot), SMRT_OFF(host_interface_values), SMRT_OFF(host_phase_samples)};
#undef SMRT_OFF
    return solver_host::copy_table(desc, out, capacity);
}

int32_t smrt_first_order_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const smrt_first_order_extras* x,
                                      const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = solver_refusals::first_order(b, x);
    if (why) { ctx->err = why; return -1; }
    if (solver_host::check_pairs(ctx, pairs, &n_pairs, (int64_t)b->n_snowpacks * b->n_frequencies)) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->first_order) ctx->first_order = new FirstOrderState();
    FirstOrderState* st = ctx->first_order;
    st->uploaded = false;
    FoBatch d = solver_describe::first_order(b, x, n_pairs);
    const solver_describe::FoExtents n = solver_describe::extents(d);
    using solver_host::upload;
    if (solver_host::upload_batch(ctx, st, b, pairs, d)) return -1;
    if (upload(ctx, st->theta, b->theta, n.theta * sizeof(double), d.theta)) return -1;
    if (b->host_layer && upload(ctx, st->hostlayer, b->host_layer, n.host_layer * sizeof(double), d.host_layer)) return -1;
    if (b->host_iba_coeff && upload(ctx, st->hostcoeff, b->host_iba_coeff, n.host_coeff * sizeof(double), d.host_coeff)) return -1;
    if (x && x->host_interface_slot) {
        if (upload(ctx, st->slot, x->host_interface_slot, n.itf_slot * sizeof(int32_t), d.itf_slot) ||
            upload(ctx, st->values, x->host_interface_values, n.itf_values * sizeof(double), d.itf_values))
            return -1;
    }
    if (x && x->host_phase_samples && upload(ctx, st->phase, x->host_phase_samples, n.host_phase * sizeof(double), d.host_phase)) return -1;
    using solver_host::reserve;
    if (reserve(ctx, st->stage, n.stage, d.stage) || reserve(ctx, st->out, n.out, d.out) || reserve(ctx, st->status, n.status, d.status) ||
        reserve(ctx, st->layer, n.layer_out, d.layer_out) || reserve(ctx, st->lb, n.layer_backscatter, d.layer_backscatter) ||
        reserve(ctx, st->diag, n.diag, d.diag) || solver_host::uploads_done(ctx))
        return -1;
    st->dev = d;
    st->uploaded = true;
    st->timed = false;
    return 0;
}

int32_t smrt_first_order_launch(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    FirstOrderState* st = ctx->first_order;
    if (!st || !st->uploaded) { ctx->err = "no first-order batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const FoBatch& d = st->dev;
    const long long items_a = d.n_pairs * d.Lmax, items_b = d.n_pairs * d.n_theta;
    st->rewind();
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(first_order_layers_kernel, dim3((unsigned)((items_a + kFoThreads - 1) / kFoThreads)), dim3(kFoThreads), 0,
                       ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    hipLaunchKernelGGL(first_order_angles_kernel, dim3((unsigned)((items_b + kFoThreads - 1) / kFoThreads)), dim3(kFoThreads), 0,
                       ctx->stream, d);
    HIPCHK(hipGetLastError());
    if (solver_host::record(ctx, st)) return -1;
    st->timed = true;
    return 0;
}

int32_t smrt_first_order_sync(smrt_dort_ctx* ctx) { return solver_host::sync(ctx); }

int32_t smrt_first_order_kernel_ms(smrt_dort_ctx* ctx, double* ms2) {
    if (!ctx || !ms2) return -1;
    FirstOrderState* st = ctx->first_order;
    if (!st || !st->timed) { ctx->err = "no first-order launch to time"; return -1; }
    ms2[0] = ms2[1] = 0.0;
    if (solver_host::wait_recorded(ctx, st) || solver_host::add_elapsed(ctx, st, 0, 1, &ms2[0]) || solver_host::add_elapsed(ctx, st, 1, 2, &ms2[1])) return -1;
    return 0;
}

int32_t smrt_first_order_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* backscatter_layer,
                                  double* diag) {
    if (!ctx) return -1;
    FirstOrderState* st = ctx->first_order;
    if (!st || !st->uploaded) { ctx->err = "no first-order batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const FoBatch& d = st->dev;
    const solver_describe::FoExtents n = solver_describe::extents(d);
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, n.out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, n.status * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.layer_out, n.layer_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (backscatter_layer)
        HIPCHK(hipMemcpyAsync(backscatter_layer, d.layer_backscatter, n.layer_backscatter * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (diag) HIPCHK(hipMemcpyAsync(diag, d.diag, n.diag * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_first_order_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_first_order_extras* extras,
                                   const int64_t* pairs, int64_t n_pairs, double* out, int32_t* status, double* layer_out,
                                   double* backscatter_layer, double* diag) {
    if (smrt_first_order_upload_pairs(ctx, batch, extras, pairs, n_pairs)) return -1;
    if (smrt_first_order_launch(ctx)) return -1;
    return smrt_first_order_download(ctx, out, status, layer_out, backscatter_layer, diag);
}

}  // extern "C"
