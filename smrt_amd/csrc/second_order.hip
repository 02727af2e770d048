// The iterative second-order backscatter solver of libsmrt_dort.so (include/smrt_dort.h: smrt_second_order_*).  Orders 0
// and 1 are the first-order solver's own upload and kernels (first_order.hip), run with the carry hook; this file adds the
// order-2 kernels -- stream sets per (pair, layer), one wavefront per integral unit, the walk per (pair, angle); arithmetic
// in second_order_kernel.hpp -- and the host side: chunks of pairs sized against the workspace budget, upload / launch /
// sync / download and the one-shot call.  An upload here replaces the resident batch of the first-order solver
// (smrt_launch::first_order_resident hands it over).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "dort_ctx.hpp"
#include "dort_host_common.hpp"
#include "second_order_kernel.hpp"
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

constexpr int kSo2Threads = 256;                       // four wavefronts = four integral units per workgroup
constexpr int kSo2UnitsPerBlock = kSo2Threads / SMRT_LANES;
constexpr int64_t kSo2DefaultBudget = 8LL << 30;

__global__ void __launch_bounds__(kSo2Threads) second_order_streams_kernel(So2Batch b) {
    const long long idx = (long long)blockIdx.x * kSo2Threads + threadIdx.x;
    if (idx >= b.chunk_count * b.fo.Lmax) return;
    second_order_stream_item(b, idx / b.fo.Lmax, (int)(idx % b.fo.Lmax));
}

// units: (row, layer, angle), angles fastest; INTER: (row, layer n, layer m, angle)
template <int M, bool INTER>
__global__ void __launch_bounds__(kSo2Threads) second_order_integrals_kernel(So2Batch b) {
    const long long unit = (long long)blockIdx.x * kSo2UnitsPerBlock + threadIdx.x / SMRT_LANES;
    const long long L = b.fo.Lmax, T = b.fo.n_theta;
    const long long units = b.chunk_count * L * T * (INTER ? L : 1);
    if (unit >= units) return;   // wavefront-uniform
    const int t = (int)(unit % T);
    long long rest = unit / T;
    int m = -1;
    if (INTER) { m = (int)(rest % L); rest /= L; }
    const int n = (int)(rest % L);
    second_order_integral_unit<M>(b, rest / L, n, m, t, threadIdx.x % SMRT_LANES);
}

__global__ void __launch_bounds__(kSo2Threads) second_order_walk_kernel(So2Batch b) {
    const long long idx = (long long)blockIdx.x * kSo2Threads + threadIdx.x;
    if (idx >= b.chunk_count * b.fo.n_theta) return;
    second_order_walk_item(b, idx / b.fo.n_theta, (int)(idx % b.fo.n_theta));
}

struct SecondOrderState {
    DevBuf gl, submodes, carry, out, lb, nstream, streams, integ;
    So2Batch dev{};
    long long chunk_rows = 0;
    bool uploaded = false, timed = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

namespace smrt_launch {
void second_order_release(smrt_dort_ctx* ctx) {
    SecondOrderState* st = ctx->second_order;
    if (!st) return;
    DevBuf* bufs[] = {&st->gl, &st->submodes, &st->carry, &st->out, &st->lb, &st->nstream, &st->streams, &st->integ};
    for (DevBuf* b : bufs) b->release();
    for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
    delete st;
    ctx->second_order = nullptr;
}
}  // namespace smrt_launch

static const char* so2_validate(const smrt_batch* b) {
    if (!b) return "null batch";
    if (b->n_max_stream < 2 || b->n_max_stream > 1024) return "n_max_stream must be 2 to 1024";
    if (b->m_max < 1 || b->m_max > kSo2MaxModes) return "m_max must be 1 to 8";
    if (!b->layer_kind && b->emmodel == SMRT_EM_HOST) return "the iterative second-order solver has no route for emmodels evaluated by the caller (SMRT_EM_HOST)";
    for (int s = 0; b->layer_kind && b->n_layers && s < b->n_snowpacks; ++s)
        for (int l = 0; l < b->n_layers[s] && l < b->n_layers_max; ++l)
            if ((b->layer_kind[(long long)s * b->n_layers_max + l] & 15) == SMRT_EM_HOST)
                return "the iterative second-order solver has no route for emmodels evaluated by the caller (SMRT_EM_HOST)";
    return nullptr;
}

template <int M>
static void so2_launch_integrals(const So2Batch& d, hipStream_t stream) {
    const long long units = d.chunk_count * d.fo.Lmax * d.fo.n_theta;
    hipLaunchKernelGGL((second_order_integrals_kernel<M, false>), dim3((unsigned)((units + kSo2UnitsPerBlock - 1) / kSo2UnitsPerBlock)),
                       dim3(kSo2Threads), 0, stream, d);
    if (d.interlayer && d.fo.Lmax > 1) {
        const long long pairs = units * d.fo.Lmax;
        hipLaunchKernelGGL((second_order_integrals_kernel<M, true>), dim3((unsigned)((pairs + kSo2UnitsPerBlock - 1) / kSo2UnitsPerBlock)),
                           dim3(kSo2Threads), 0, stream, d);
    }
}

extern "C" {

int32_t smrt_second_order_out_stride(const smrt_batch* b) { return b ? 28 * b->n_theta : -1; }

int32_t smrt_second_order_abi(int32_t* out, int32_t capacity) {
#define SMRT_OFF(f) (int32_t)offsetof(smrt_second_order_extras, f)
    const int32_t desc[] = {(int32_t)sizeof(smrt_second_order_extras), SMRT_OFF(compute_scattering_interlayer), SMRT_OFF(reserved),
                            SMRT_OFF(workspace_budget_bytes), SMRT_OFF(first_order), SMRT_OFF(substrate_diffuse_modes)};
#undef SMRT_OFF
    const int32_t n = (int32_t)(sizeof(desc) / sizeof(desc[0]));
    for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = desc[i];
    return n;
}

int32_t smrt_second_order_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const smrt_second_order_extras* x,
                                       const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = so2_validate(b);
    if (why) { ctx->err = why; return -1; }
    if (ctx->second_order) ctx->second_order->uploaded = false;
    // inputs, staging rows and first-order outputs: the first-order solver's own upload (it validates the rest)
    if (smrt_first_order_upload_pairs(ctx, b, x ? x->first_order : nullptr, pairs, n_pairs)) return -1;
    if (!ctx->second_order) {
        ctx->second_order = new SecondOrderState();
        for (hipEvent_t& e : ctx->second_order->ev) HIPCHK(hipEventCreate(&e));
    }
    SecondOrderState* st = ctx->second_order;
    FoBatch* fo = smrt_launch::first_order_resident(ctx);
    if (!fo) { ctx->err = "no first-order batch resident"; return -1; }
    const size_t N = (size_t)fo->n_pairs, L = b->n_layers_max, T = b->n_theta, NM = b->n_max_stream, MM = b->m_max;
    const size_t FS = (size_t)b->n_frequencies * b->n_snowpacks;
    So2Batch d{};
    d.nmax = (int)NM; d.m_max = (int)MM; d.nsamp = azimuth_samples(b->m_max);
    d.interlayer = (x && x->compute_scattering_interlayer) ? 1 : 0;
    const int64_t budget = (x && x->workspace_budget_bytes > 0) ? x->workspace_budget_bytes : kSo2DefaultBudget;
    const size_t sub_bytes = (x && x->substrate_diffuse_modes) ? FS * L * T * NM * MM * kSo2SubDoubles * sizeof(double) : 0;
    const size_t fixed = NM * 8 + sub_bytes + N * L * T * kFoCarryDoubles * 8 + N * 28 * T * 8 + N * (L + 1) * T * 4 * 8;
    const size_t slots = 2 + (d.interlayer ? L : 0);
    const size_t per_row = L * 4 + L * 2 * NM * 8 + L * T * slots * 4 * 8;
    if ((int64_t)(fixed + per_row) > budget) {
        ctx->err = "the workspace budget of the iterative second-order solver is smaller than the buffers of the batch itself plus one pair (" +
                   std::to_string(fixed + per_row) + " bytes)";
        return -1;
    }
    st->chunk_rows = (long long)std::min<size_t>(N, (size_t)(budget - (int64_t)fixed) / per_row);
    std::vector<double> gl(NM);
    smrt_host::gauss_legendre_positive((int)NM, gl.data(), nullptr);
    HIPCHK(st->gl.reserve(NM * sizeof(double)));
    HIPCHK(hipMemcpyAsync(st->gl.p, gl.data(), NM * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (sub_bytes) {
        HIPCHK(st->submodes.reserve(sub_bytes));
        HIPCHK(hipMemcpyAsync(st->submodes.p, x->substrate_diffuse_modes, sub_bytes, hipMemcpyHostToDevice, ctx->stream));
        d.sub_modes = (const double*)st->submodes.p;
    }
    HIPCHK(st->carry.reserve(N * L * T * kFoCarryDoubles * sizeof(double)));
    HIPCHK(st->out.reserve(N * 28 * T * sizeof(double)));
    HIPCHK(st->lb.reserve(N * (L + 1) * T * 4 * sizeof(double)));
    const size_t R = (size_t)st->chunk_rows;
    HIPCHK(st->nstream.reserve(R * L * sizeof(int32_t)));
    HIPCHK(st->streams.reserve(R * L * 2 * NM * sizeof(double)));
    HIPCHK(st->integ.reserve(R * L * T * slots * 4 * sizeof(double)));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // gl is this function's own vector; the caller's modes may go away
    fo->carry = (double*)st->carry.p;
    d.fo = *fo;
    d.gl_mu = (const double*)st->gl.p;
    d.nstream = (int*)st->nstream.p; d.streams = (double*)st->streams.p; d.integ = (double*)st->integ.p;
    d.out = (double*)st->out.p; d.layer_backscatter = (double*)st->lb.p;
    st->dev = d;
    st->uploaded = true;
    st->timed = false;
    return 0;
}

int32_t smrt_second_order_launch(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    SecondOrderState* st = ctx->second_order;
    const FoBatch* fo = smrt_launch::first_order_resident(ctx);
    if (!st || !st->uploaded || !fo || fo->carry != st->carry.p || !st->carry.p) {
        ctx->err = "no second-order batch uploaded";
        return -1;
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventRecord(st->ev[0], ctx->stream));
    if (smrt_first_order_launch(ctx)) return -1;   // layer scalars, orders 0 and 1, the carry
    HIPCHK(hipEventRecord(st->ev[1], ctx->stream));
    So2Batch d = st->dev;
    const long long N = d.fo.n_pairs, L = d.fo.Lmax, T = d.fo.n_theta;
    for (long long begin = 0; begin < N; begin += st->chunk_rows) {
        d.chunk_begin = begin;
        d.chunk_count = std::min(st->chunk_rows, N - begin);
        hipLaunchKernelGGL(second_order_streams_kernel, dim3((unsigned)((d.chunk_count * L + kSo2Threads - 1) / kSo2Threads)),
                           dim3(kSo2Threads), 0, ctx->stream, d);
        HIPCHK(hipGetLastError());
        if (d.m_max <= 2) so2_launch_integrals<2>(d, ctx->stream);
        else if (d.m_max <= 3) so2_launch_integrals<3>(d, ctx->stream);
        else if (d.m_max <= 5) so2_launch_integrals<5>(d, ctx->stream);
        else so2_launch_integrals<8>(d, ctx->stream);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(second_order_walk_kernel, dim3((unsigned)((d.chunk_count * T + kSo2Threads - 1) / kSo2Threads)),
                           dim3(kSo2Threads), 0, ctx->stream, d);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(st->ev[2], ctx->stream));
    st->timed = true;
    return 0;
}

int32_t smrt_second_order_sync(smrt_dort_ctx* ctx) { return smrt_first_order_sync(ctx); }

int32_t smrt_second_order_kernel_ms(smrt_dort_ctx* ctx, double* ms2) {
    if (!ctx || !ms2) return -1;
    SecondOrderState* st = ctx->second_order;
    if (!st || !st->timed) { ctx->err = "no second-order launch to time"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(st->ev[2]));
    float a = 0.f, c = 0.f;
    HIPCHK(hipEventElapsedTime(&a, st->ev[0], st->ev[1]));
    HIPCHK(hipEventElapsedTime(&c, st->ev[1], st->ev[2]));
    ms2[0] = a; ms2[1] = c;
    return 0;
}

int32_t smrt_second_order_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* backscatter_layer,
                                   double* diag) {
    if (!ctx) return -1;
    SecondOrderState* st = ctx->second_order;
    if (!st || !st->uploaded) { ctx->err = "no second-order batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const So2Batch& d = st->dev;
    const size_t N = (size_t)d.fo.n_pairs, L = d.fo.Lmax, T = d.fo.n_theta;
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, N * 28 * T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (backscatter_layer)
        HIPCHK(hipMemcpyAsync(backscatter_layer, d.layer_backscatter, N * (L + 1) * T * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return smrt_first_order_download(ctx, nullptr, status, layer_out, nullptr, diag);   // synchronises the stream
}

int32_t smrt_second_order_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_second_order_extras* extras,
                                    const int64_t* pairs, int64_t n_pairs, double* out, int32_t* status, double* layer_out,
                                    double* backscatter_layer, double* diag) {
    if (smrt_second_order_upload_pairs(ctx, batch, extras, pairs, n_pairs)) return -1;
    if (smrt_second_order_launch(ctx)) return -1;
    return smrt_second_order_download(ctx, out, status, layer_out, backscatter_layer, diag);
}

}  // extern "C"
