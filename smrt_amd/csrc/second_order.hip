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

#include "solver_describe.hpp"
#include "solver_host.hpp"
#include "solver_refusals.hpp"

using namespace smrt;

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

struct SecondOrderState : solver_host::SolverState {
    DevBuf &gl = buf(), &submodes = buf(), &carry = buf(), &out = buf(), &lb = buf(), &nstream = buf(), &streams = buf(), &integ = buf();
    So2Batch dev{};
    long long chunk_rows = 0;
    bool uploaded = false, timed = false;   // events 0, 1, 2 around the first-order launch and the chunks of the last launch
};

namespace smrt_launch {
void second_order_release(smrt_dort_ctx* ctx) { solver_host::release(ctx->second_order); }
}  // namespace smrt_launch

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
    return solver_host::copy_table(desc, out, capacity);
}

int32_t smrt_second_order_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const smrt_second_order_extras* x,
                                       const int64_t* pairs, int64_t n_pairs) {
    if (!ctx) return -1;
    const char* why = solver_refusals::second_order(b);
    if (why) { ctx->err = why; return -1; }
    if (ctx->second_order) ctx->second_order->uploaded = false;
    // inputs, staging rows and first-order outputs: the first-order solver's own upload (it validates the rest)
    if (smrt_first_order_upload_pairs(ctx, b, x ? x->first_order : nullptr, pairs, n_pairs)) return -1;
    if (!ctx->second_order) ctx->second_order = new SecondOrderState();
    SecondOrderState* st = ctx->second_order;
    FoBatch* fo = smrt_launch::first_order_resident(ctx);
    if (!fo) { ctx->err = "no first-order batch resident"; return -1; }
    So2Batch d = solver_describe::second_order(b, x, fo->n_pairs);
    const size_t N = (size_t)fo->n_pairs, NM = d.nmax, carry_doubles = solver_describe::extents(*fo).carry;
    const solver_describe::So2Extents row = solver_describe::extents(d, 1);
    const int64_t budget = (x && x->workspace_budget_bytes > 0) ? x->workspace_budget_bytes : kSo2DefaultBudget;
    const size_t sub_bytes = (x && x->substrate_diffuse_modes) ? row.sub_modes * sizeof(double) : 0;
    const size_t fixed = (row.gl_mu + carry_doubles + row.out + row.layer_backscatter) * sizeof(double) + sub_bytes;
    const size_t per_row = row.nstream * sizeof(int32_t) + (row.streams + row.integ) * sizeof(double);
    if ((int64_t)(fixed + per_row) > budget) {
        ctx->err = "the workspace budget of the iterative second-order solver is smaller than the buffers of the batch itself plus one pair (" +
                   std::to_string(fixed + per_row) + " bytes)";
        return -1;
    }
    st->chunk_rows = (long long)std::min<size_t>(N, (size_t)(budget - (int64_t)fixed) / per_row);
    std::vector<double> gl(NM);
    smrt_host::gauss_legendre_positive((int)NM, gl.data(), nullptr);
    if (solver_host::upload(ctx, st->gl, gl.data(), NM * sizeof(double), d.gl_mu)) return -1;
    if (sub_bytes && solver_host::upload(ctx, st->submodes, x->substrate_diffuse_modes, sub_bytes, d.sub_modes)) return -1;
    const solver_describe::So2Extents n = solver_describe::extents(d, (size_t)st->chunk_rows);
    HIPCHK(st->carry.reserve(carry_doubles * sizeof(double)));
    HIPCHK(st->out.reserve(n.out * sizeof(double)));
    HIPCHK(st->lb.reserve(n.layer_backscatter * sizeof(double)));
    HIPCHK(st->nstream.reserve(n.nstream * sizeof(int32_t)));
    HIPCHK(st->streams.reserve(n.streams * sizeof(double)));
    HIPCHK(st->integ.reserve(n.integ * sizeof(double)));
    if (solver_host::uploads_done(ctx)) return -1;
    fo->carry = (double*)st->carry.p;
    d.fo = *fo;
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
    st->rewind();
    if (solver_host::record(ctx, st)) return -1;
    if (smrt_first_order_launch(ctx)) return -1;   // layer scalars, orders 0 and 1, the carry
    if (solver_host::record(ctx, st)) return -1;
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
    if (solver_host::record(ctx, st)) return -1;
    st->timed = true;
    return 0;
}

int32_t smrt_second_order_sync(smrt_dort_ctx* ctx) { return solver_host::sync(ctx); }

int32_t smrt_second_order_kernel_ms(smrt_dort_ctx* ctx, double* ms2) {
    if (!ctx || !ms2) return -1;
    SecondOrderState* st = ctx->second_order;
    if (!st || !st->timed) { ctx->err = "no second-order launch to time"; return -1; }
    ms2[0] = ms2[1] = 0.0;
    if (solver_host::wait_recorded(ctx, st) || solver_host::add_elapsed(ctx, st, 0, 1, &ms2[0]) || solver_host::add_elapsed(ctx, st, 1, 2, &ms2[1])) return -1;
    return 0;
}

int32_t smrt_second_order_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* backscatter_layer,
                                   double* diag) {
    if (!ctx) return -1;
    SecondOrderState* st = ctx->second_order;
    if (!st || !st->uploaded) { ctx->err = "no second-order batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const So2Batch& d = st->dev;
    const solver_describe::So2Extents n = solver_describe::extents(d, (size_t)st->chunk_rows);
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, n.out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (backscatter_layer)
        HIPCHK(hipMemcpyAsync(backscatter_layer, d.layer_backscatter, n.layer_backscatter * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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
