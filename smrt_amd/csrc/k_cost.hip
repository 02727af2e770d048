// Work estimate per pair for cost-weighted sharding: sum over the layers (and azimuth modes) of N_l^3
// with the actual stream counts, from the first stage of the solve only (layer permittivities -> streams per layer).
// The same stream counts give every item's size class of rows: the count and fill steps of dort_class_lists.hpp.
#include "dort_ctx.hpp"
#include "dort_device.hpp"

using namespace smrt;

template <int NT>
__global__ __launch_bounds__(NT) void dort_cost_kernel(DevBatch b, double* cost, int* class_rows, int* class_counts) {
    extern __shared__ __attribute__((aligned(16))) double smrt_lds[];
    dort_cost_pair<NT>(b, (long long)blockIdx.x, smrt_lds, cost, class_rows, class_counts);
}

// one thread per dispatch position of the upload (class_fill_pair)
__global__ __launch_bounds__(256) void dort_class_fill_kernel(int Lmax, long long pair_count, long long chunk_pairs, const int* dispatch,
                                                              const int* rows, const long long* pair_offset, int* list) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w < pair_count) class_fill_pair(Lmax, chunk_pairs, dispatch, rows, pair_offset, w, list);
}

// see prune_mark_pair (dort_passive.hpp): one wavefront per pair
__global__ __launch_bounds__(64) void dort_prune_mark_kernel(DevBatch b, DevStage stg, int* done) {
    prune_mark_pair(b, stg, (long long)blockIdx.x, done);
}

namespace smrt_launch {
hipError_t prune_mark(smrt_dort_ctx* ctx, const DevBatch& c, int* done_dev) {
    hipLaunchKernelGGL(dort_prune_mark_kernel, dim3((unsigned)c.pair_count), dim3(64), 0, ctx->stream, c, ctx->stage, done_dev);
    return hipGetLastError();
}
hipError_t pair_cost(smrt_dort_ctx* ctx, const DevBatch& d, double* cost_dev, int* class_rows_dev, int* class_counts_dev) {
    const int P = d.mode == 1 ? 3 : 2;
    const size_t lds = (size_t)make_plan(d.n_max_stream, P, d.Lmax, d.n_theta, 1, 0, 0, 1).total * sizeof(double);
    auto kern = dort_cost_kernel<64>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)d.pair_count), dim3(64), lds, ctx->stream, d, cost_dev, class_rows_dev, class_counts_dev);
    return hipGetLastError();
}
hipError_t class_fill(smrt_dort_ctx* ctx, const DevBatch& d, long long chunk_pairs, const int* rows_dev, const long long* pair_offset_dev, int* list_dev) {
    hipLaunchKernelGGL(dort_class_fill_kernel, dim3((unsigned)((d.pair_count + 255) / 256)), dim3(256), 0, ctx->stream, d.Lmax, d.pair_count, chunk_pairs,
                       d.dispatch, rows_dev, pair_offset_dev, list_dev);
    return hipGetLastError();
}
}  // namespace smrt_launch
