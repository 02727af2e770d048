// The iterative first-order backscatter solver of libsmrt_dort.so (include/smrt_dort.h: smrt_first_order_*): its two
// kernels -- one lane per (pair, layer) for the layer electromagnetics, one lane per (pair, incidence angle) for the
// recursion; arithmetic in first_order_kernel.hpp -- and the host side: buffers on the DORT context, upload / launch /
// sync / download and the one-shot call.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>
#include <string>

#include "dort_ctx.hpp"
#include "first_order_kernel.hpp"
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

struct FirstOrderState {
    DevBuf nl, thick, fv, temp, p1, p2, freq, theta, lw, kind, hostlayer, hostcoeff, sub1, sub2, pairmap, slot, values, phase;
    DevBuf stage, out, status, layer, lb, diag;
    FoBatch dev{};
    bool uploaded = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timed = false;
};

namespace smrt_launch {
void first_order_release(smrt_dort_ctx* ctx) {
    FirstOrderState* st = ctx->first_order;
    if (!st) return;
    DevBuf* bufs[] = {&st->nl, &st->thick, &st->fv, &st->temp, &st->p1, &st->p2, &st->freq, &st->theta, &st->lw, &st->kind,
                      &st->hostlayer, &st->hostcoeff, &st->sub1, &st->sub2, &st->pairmap, &st->slot, &st->values, &st->phase,
                      &st->stage, &st->out, &st->status, &st->layer, &st->lb, &st->diag};
    for (DevBuf* b : bufs) b->release();
    for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
    delete st;
    ctx->first_order = nullptr;
}
FoBatch* first_order_resident(smrt_dort_ctx* ctx) {
    FirstOrderState* st = ctx->first_order;
    return st && st->uploaded ? &st->dev : nullptr;
}
}  // namespace smrt_launch

static int fo_upload(smrt_dort_ctx* ctx, DevBuf& buf, const void* src, size_t bytes) {
    HIPCHK(buf.reserve(bytes));
    HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

static const char* fo_validate(const smrt_batch* b, const smrt_first_order_extras* x) {
    if (!b) return "null batch";
    if (b->n_snowpacks <= 0 || b->n_frequencies <= 0 || b->n_layers_max <= 0) return "empty batch";
    if (b->n_theta <= 0) return "n_theta must be positive";
    if (b->mode != SMRT_MODE_ACTIVE) return "the iterative first-order solver needs an active sensor";
    if (b->emmodel < SMRT_EM_IBA || b->emmodel > SMRT_EM_RAYLEIGH_HOST) return "unknown emmodel";
    if (b->microstructure < SMRT_MS_EXPONENTIAL || b->microstructure > SMRT_MS_TEUBNER_STREY) return "unknown microstructure";
    if (!b->n_layers || !b->thickness || !b->frac_volume || !b->temperature || !b->micro_p1 || !b->frequency || !b->theta)
        return "null input array";
    if ((b->microstructure == SMRT_MS_STICKY_HARD_SPHERES || b->layer_kind) && !b->micro_p2) return "stickiness array missing";
    bool host_scalars = !b->layer_kind && b->emmodel >= SMRT_EM_HOST && b->emmodel != SMRT_EM_IBA_INVERTED;
    bool iba_host = !b->layer_kind && b->emmodel == SMRT_EM_IBA_HOST;
    bool dmrt = !b->layer_kind && (b->emmodel == SMRT_EM_DMRT_QCA_SHORTRANGE || b->emmodel == SMRT_EM_DMRT_QCACP_SHORTRANGE);
    if (dmrt && b->microstructure != SMRT_MS_STICKY_HARD_SPHERES)
        return "the dmrt short-range emmodels are only compatible with sticky_hard_spheres";
    for (int s = 0; s < b->n_snowpacks; ++s) {
        if (b->n_layers[s] < 1 || b->n_layers[s] > b->n_layers_max) return "n_layers out of range";
        for (int l = 0; b->layer_kind && l < b->n_layers[s]; ++l) {
            const int k = b->layer_kind[(long long)s * b->n_layers_max + l], em = k & 15, ms = k >> 4;
            if (em < SMRT_EM_IBA || em > SMRT_EM_RAYLEIGH_HOST || ms < SMRT_MS_EXPONENTIAL || ms > SMRT_MS_TEUBNER_STREY)
                return "invalid layer_kind entry";
            if ((em == SMRT_EM_DMRT_QCA_SHORTRANGE || em == SMRT_EM_DMRT_QCACP_SHORTRANGE) && ms != SMRT_MS_STICKY_HARD_SPHERES)
                return "the dmrt short-range emmodels are only compatible with sticky_hard_spheres";
            if (em == SMRT_EM_HOST || em == SMRT_EM_IBA_HOST || em == SMRT_EM_RAYLEIGH_HOST) host_scalars = true;
            if (em == SMRT_EM_IBA_HOST) iba_host = true;
        }
    }
    if (host_scalars && !b->host_layer) return "layers evaluated by the caller need host_layer";
    if (iba_host && !b->host_iba_coeff) return "layers of kind SMRT_EM_IBA_HOST need host_iba_coeff";
    if (b->substrate_kind < SMRT_SUBSTRATE_NONE || b->substrate_kind > SMRT_SUBSTRATE_REFLECTOR)
        return "substrate_kind must be none, flat or reflector: any other substrate travels in smrt_first_order_extras";
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE && (!b->substrate_p1 || !b->substrate_p2)) return "substrate arrays missing";
    if (x && x->host_interface_slot) {
        if (x->n_interface_slots < 1 || !x->host_interface_values) return "host_interface_slot needs host_interface_values and n_interface_slots >= 1";
        const long long n = (long long)b->n_frequencies * b->n_snowpacks * (b->n_layers_max + 1);
        for (long long i = 0; i < n; ++i)
            if (x->host_interface_slot[i] < -1 || x->host_interface_slot[i] >= x->n_interface_slots) return "host_interface_slot entry out of range";
    }
    return nullptr;
}

extern "C" {

int32_t smrt_first_order_out_stride(const smrt_batch* b) { return b ? 16 * b->n_theta : -1; }

int32_t smrt_first_order_abi(int32_t* out, int32_t capacity) {
#define SMRT_OFF(f) (int32_t)offsetof(smrt_first_order_extras, f)
    const int32_t desc[] = {(int32_t)sizeof(smrt_first_order_extras), SMRT_OFF(n_interface_slots), SMRT_OFF(reserved),
                            SMRT_OFF(host_interface_slot), SMRT_OFF(host_interface_values), SMRT_OFF(host_phase_samples)};
#undef SMRT_OFF
    const int32_t n = (int32_t)(sizeof(desc) / sizeof(desc[0]));
    for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = desc[i];
    return n;
}

int32_t smrt_first_order_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const smrt_first_order_extras* x,
                                      const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = fo_validate(b, x);
    if (why) { ctx->err = why; return -1; }
    const int64_t all = (int64_t)b->n_snowpacks * b->n_frequencies;
    if (!pairs) n_pairs = all;
    else {
        if (n_pairs <= 0) { ctx->err = "empty pair list"; return -1; }
        for (int64_t i = 0; i < n_pairs; ++i)
            if (pairs[i] < 0 || pairs[i] >= all) { ctx->err = "pair index out of bounds"; return -1; }
    }
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->first_order) {
        ctx->first_order = new FirstOrderState();
        for (hipEvent_t& e : ctx->first_order->ev) HIPCHK(hipEventCreate(&e));
    }
    FirstOrderState* st = ctx->first_order;
    st->uploaded = false;
    const size_t S = b->n_snowpacks, L = b->n_layers_max, F = b->n_frequencies, T = b->n_theta, N = (size_t)n_pairs;
    const size_t SL = S * L * sizeof(double), FS = F * S;
    FoBatch d{};
    d.S = (int)S; d.Lmax = (int)L; d.F = (int)F; d.n_theta = (int)T;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.sub_kind = b->substrate_kind;
    d.n_pairs = n_pairs;
#define FO_UP(buf, src, bytes, field) do { if (fo_upload(ctx, st->buf, src, bytes)) return -1; d.field = (decltype(d.field))st->buf.p; } while (0)
    FO_UP(nl, b->n_layers, S * sizeof(int32_t), n_layers);
    FO_UP(thick, b->thickness, SL, thickness);
    FO_UP(fv, b->frac_volume, SL, frac_volume);
    FO_UP(temp, b->temperature, SL, temperature);
    FO_UP(p1, b->micro_p1, SL, p1);
    if (b->micro_p2) FO_UP(p2, b->micro_p2, SL, p2);
    FO_UP(freq, b->frequency, F * sizeof(double), frequency);
    FO_UP(theta, b->theta, T * sizeof(double), theta);
    if (b->liquid_water) FO_UP(lw, b->liquid_water, SL, liquid_water);
    if (b->layer_kind) FO_UP(kind, b->layer_kind, S * L * sizeof(int32_t), layer_kind);
    if (b->host_layer) FO_UP(hostlayer, b->host_layer, FS * L * 4 * sizeof(double), host_layer);
    if (b->host_iba_coeff) FO_UP(hostcoeff, b->host_iba_coeff, FS * L * sizeof(double), host_coeff);
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE) {
        FO_UP(sub1, b->substrate_p1, FS * sizeof(double), sub_p1);
        FO_UP(sub2, b->substrate_p2, FS * sizeof(double), sub_p2);
    }
    if (pairs) FO_UP(pairmap, pairs, N * sizeof(int64_t), pair_map);
    if (x && x->host_interface_slot) {
        d.n_slots = x->n_interface_slots;
        FO_UP(slot, x->host_interface_slot, FS * (L + 1) * sizeof(int32_t), itf_slot);
        FO_UP(values, x->host_interface_values, FS * (size_t)d.n_slots * T * kFoInterfaceDoubles * sizeof(double), itf_values);
    }
    if (x && x->host_phase_samples) FO_UP(phase, x->host_phase_samples, FS * L * T * 16 * sizeof(double), host_phase);
#undef FO_UP
    HIPCHK(st->stage.reserve((size_t)FO_ROWS * L * N * sizeof(double)));
    HIPCHK(st->out.reserve(N * 16 * T * sizeof(double)));
    HIPCHK(st->status.reserve(N * sizeof(int32_t)));
    HIPCHK(st->layer.reserve(N * L * 5 * sizeof(double)));
    HIPCHK(st->lb.reserve(N * (L + 1) * T * 4 * sizeof(double)));
    HIPCHK(st->diag.reserve(N * 2 * sizeof(double)));
    d.stage = (double*)st->stage.p; d.out = (double*)st->out.p; d.status = (int*)st->status.p;
    d.layer_out = (double*)st->layer.p; d.layer_backscatter = (double*)st->lb.p; d.diag = (double*)st->diag.p;
    // the copies above read the caller's (pageable) arrays: wait for them, the arrays may go away or change after this call
    HIPCHK(hipStreamSynchronize(ctx->stream));
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
    HIPCHK(hipEventRecord(st->ev[0], ctx->stream));
    hipLaunchKernelGGL(first_order_layers_kernel, dim3((unsigned)((items_a + kFoThreads - 1) / kFoThreads)), dim3(kFoThreads), 0,
                       ctx->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[1], ctx->stream));
    hipLaunchKernelGGL(first_order_angles_kernel, dim3((unsigned)((items_b + kFoThreads - 1) / kFoThreads)), dim3(kFoThreads), 0,
                       ctx->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st->ev[2], ctx->stream));
    st->timed = true;
    return 0;
}

int32_t smrt_first_order_sync(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_first_order_kernel_ms(smrt_dort_ctx* ctx, double* ms2) {
    if (!ctx || !ms2) return -1;
    FirstOrderState* st = ctx->first_order;
    if (!st || !st->timed) { ctx->err = "no first-order launch to time"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(st->ev[2]));
    float a = 0.f, c = 0.f;
    HIPCHK(hipEventElapsedTime(&a, st->ev[0], st->ev[1]));
    HIPCHK(hipEventElapsedTime(&c, st->ev[1], st->ev[2]));
    ms2[0] = a; ms2[1] = c;
    return 0;
}

int32_t smrt_first_order_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* backscatter_layer,
                                  double* diag) {
    if (!ctx) return -1;
    FirstOrderState* st = ctx->first_order;
    if (!st || !st->uploaded) { ctx->err = "no first-order batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const FoBatch& d = st->dev;
    const size_t N = (size_t)d.n_pairs, L = d.Lmax, T = d.n_theta;
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, N * 16 * T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, N * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.layer_out, N * L * 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (backscatter_layer)
        HIPCHK(hipMemcpyAsync(backscatter_layer, d.layer_backscatter, N * (L + 1) * T * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (diag) HIPCHK(hipMemcpyAsync(diag, d.diag, N * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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
