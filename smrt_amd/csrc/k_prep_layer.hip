// Kernels of the per-layer prep of the LDS-resident passive pipelines (N <= 64): pair setup and one layer kernel per size
// class of rows, see dort_prep_layer.hpp.
// hipcc-flags: -mllvm -disable-machine-licm
// (as for the per-pair prep kernel in k_split_passive.hip: fewer loop-invariant values hoisted and spilled)
#include <cstdlib>
#include "dort_ctx.hpp"
#include "dort_device.hpp"
#include "dort_prep_layer.hpp"

using namespace smrt;

__global__ __launch_bounds__(64) void dort_prep_setup_kernel(DevBatch b, DevStage st) {
    extern __shared__ __attribute__((aligned(16))) double smrt_lds[];
    dort_prep_setup_pair<64>(b, dispatched_pair(b, (long long)blockIdx.x), smrt_lds, st);
}

// One workgroup per item of the launch -- the chunk's list of the class (dort_class_lists.hpp), or all the items of the round,
// like the eigensolver's kernels; an item outside the class (LO, HI] leaves at once.  WAVES: wavefronts per SIMD the compiler leaves room for -- what the LDS of the class lets in.
template <int NT, int LO, int HI, int WAVES>
__global__ __launch_bounds__(NT, WAVES) void dort_prep_layer_kernel(DevBatch b, DevStage st) {
    extern __shared__ __attribute__((aligned(16))) double smrt_lds[];
    const long long item = class_item_of_block(b, (long long)blockIdx.x);
    const int rows = prep_item_rows(b, st, item);
    if (rows <= LO || rows > HI) { class_list_left(b, rows); return; }
    dort_prep_layer_item<NT, HI>(b, st, item, smrt_lds);
}

namespace smrt_launch {

template <int NT, int LO, int HI, int WAVES>
static hipError_t go_layer(smrt_dort_ctx* ctx, const DevBatch& c, long long items, const ClassSegments* seg) {
    DevBatch cl = c;
    if (!class_launch<LO, HI>(cl, items, seg)) return hipSuccess;
    const size_t lds = sizeof(double) * (size_t)make_plan(HI / 2, 2, 0, 0, 9, 1, 0, 4).total;
    hipError_t e = hipFuncSetAttribute((const void*)dort_prep_layer_kernel<NT, LO, HI, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((dort_prep_layer_kernel<NT, LO, HI, WAVES>), dim3((unsigned)items), dim3(NT), lds, ctx->stream, cl, ctx->stage);
    return hipGetLastError();
}

// Size classes by row count, the eigensolver's: (0, 32], (32, 48], (48, 64].  LDS 14.3 / 25.5 / 40.7 KB.
hipError_t prep_layers(smrt_dort_ctx* ctx, const DevBatch& c, long long items, const ClassSegments* seg) {
    const size_t lds = sizeof(double) * (size_t)make_plan(c.n_max_stream, 2, c.Lmax, c.n_theta, 9, 1, 0, 5).total;
    hipLaunchKernelGGL(dort_prep_setup_kernel, dim3((unsigned)c.pair_count), dim3(64), lds, ctx->stream, c, ctx->stage);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int nmax = ctx->nmax_rows;
    // (four wavefronts per SIMD for every class: the body takes 106 registers; held to the 96 of five it spills 44 bytes)
    static const bool nt128 = getenv("SMRT_DORT_PREP_LAYER_NT") && atoi(getenv("SMRT_DORT_PREP_LAYER_NT")) == 128;   // experiment switch, two smaller classes
    if (nt128) {
        if ((e = go_layer<128, 0, 32, 4>(ctx, c, items, seg)) != hipSuccess) return e;
        if (nmax > 32 && (e = go_layer<128, 32, 48, 4>(ctx, c, items, seg)) != hipSuccess) return e;
    } else {
        if ((e = go_layer<256, 0, 32, 4>(ctx, c, items, seg)) != hipSuccess) return e;
        if (nmax > 32 && (e = go_layer<256, 32, 48, 4>(ctx, c, items, seg)) != hipSuccess) return e;
    }
    if (nmax > 48 && (e = go_layer<256, 48, 64, 4>(ctx, c, items, seg)) != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace smrt_launch
