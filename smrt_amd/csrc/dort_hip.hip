// libsmrt_dort.so -- HIP implementation of include/smrt_dort.h for gfx950 (MI355X).
// This file: the C ABI, the context, device buffers, packing, the chunk loops and HIP-event timing.  The kernels are
// instantiated in k_*.hip (one translation unit per kernel family, compiled in parallel) behind the launchers of
// dort_ctx.hpp; the device code itself is dort_device.hpp and the headers it lists.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dort_ctx.hpp"
#include "dort_eig_kernel.hpp"      // eig_rot_doubles
#include "dort_rayleigh_kernel.hpp" // em_has_rayleigh_phase
#include "dort_jacobi_big.hpp"      // make_jacobi_plan, make_jacobi_big_plan (templates only: nothing is instantiated here)
#include "dort_host_common.hpp"
#include "dort_phase_kernel.hpp"
#include "dort_finish_reg.hpp"      // finish_reg_lds_doubles (device code is inline templates / functions: nothing is instantiated here)
#include "dort_finish_strip.hpp"    // finish_strip_lds_doubles
#include "solver_host.hpp"          // HIPCHK

using namespace smrt;

static int upload_array(smrt_dort_ctx* ctx, DevBuf& buf, const void* src, size_t bytes) {
    HIPCHK(buf.reserve(bytes));
    HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}


// One chunk of the batch as its own DevBatch (outputs offset to the chunk's rows)
static DevBatch chunk_of(const smrt_dort_ctx* ctx, const DevBatch& d, long long c0, long long cn) {
    DevBatch c = d;
    c.pair_begin = d.pair_begin + c0; c.pair_count = cn;
    c.out = d.out + c0 * ctx->out_stride; c.status = d.status + c0;
    c.layer_out = d.layer_out + c0 * (long long)d.Lmax * 5;
    c.stream_out = d.stream_out + c0 * (long long)(1 + d.n_max_stream);
    c.n3_out = d.n3_out + c0; c.stage_out = d.stage_out + c0 * 16;
    if (d.dispatch) c.dispatch = d.dispatch + c0;
    return c;
}

// prep -> Jacobi -> finish, chunk by chunk (the staging area holds one chunk).  Under prune_deep_snowpack the prep and
// Jacobi kernels run in up to four ROUNDS over successive layer ranges, top-down, with a small kernel in between that
// marks the pairs whose cut has been reached: the layers below a cut are never diagonalised (like in the reference),
// exactly -- the decision uses the same singular values as the finish kernel.
#ifndef SMRT_DORT_LANES_DEFAULT
#define SMRT_DORT_LANES_DEFAULT 1   // concurrent pipeline passes on the LDS pipelines (SMRT_DORT_LANES overrides; measured in profiles/)
#endif
#ifndef SMRT_PREP_DEFAULT
#define SMRT_PREP_DEFAULT SMRT_PREP_PER_LAYER   // the prep of the passive LDS pipelines (smrt_dort_set_prep / SMRT_DORT_PREP_LAYERS override)
#endif
#ifndef SMRT_FINISH_STRIP_DEFAULT
#define SMRT_FINISH_STRIP_DEFAULT 1   // the strip finish kernel where it is supported (64 < N <= 128, passive; set_pipeline(4) / SMRT_DORT_FINISH_STRIP=0: the pivoted one)
#endif
#ifndef SMRT_FINISH_REG_DEFAULT
#define SMRT_FINISH_REG_DEFAULT 1   // the register-resident finish kernel where it is supported (set_pipeline(3) / SMRT_DORT_FINISH_REG=1 force it)
#endif
static hipError_t launch_pipeline(smrt_dort_ctx* ctx, const DevBatch& d) {
    const long long items_per_pair = (long long)(ctx->active ? d.m_max + 1 : 1) * d.Lmax;
    const long long modes = ctx->active ? d.m_max + 1 : 1;
    if (getenv("SMRT_DORT_DEBUG_OCCUPANCY") && !ctx->gmem_path && !ctx->active) smrt_launch::occupancy_report(ctx, ctx->nt);
    // (under process_coherent_layers the layer indices of a pair are its own: one round, and the staging counts of the
    // removed layers must read "nothing staged")
    const int rounds = (d.prune_tau > 0.0 && !d.coherent && getenv("SMRT_DORT_NO_PRUNE_ROUNDS") == nullptr) ? std::min(4, d.Lmax) : 1;
    auto prep = [&](const DevBatch& c, unsigned grid, const ClassSegments* seg) {
        if (ctx->prep_layers) return smrt_launch::prep_layers(ctx, c, c.pair_count * (c.layer_hi - c.layer_lo), seg);
        if (ctx->big) return smrt_launch::prep_gmem_big(ctx, c, grid, ctx->active, ctx->nmax_rows <= 256 ? 4 : 6);
        if (ctx->prep_wide) return smrt_launch::prep_wide(ctx, c);
        if (ctx->gmem_split) return smrt_launch::prep_gmem(ctx, c, grid, ctx->active);
        return ctx->active ? smrt_launch::active_prep(ctx, c, ctx->nt) : smrt_launch::prep(ctx, c, ctx->nt);
    };
    auto finish = [&](const DevBatch& c, unsigned grid) {
        if (ctx->big) return smrt_launch::finish_gmem_big(ctx, c, grid, ctx->active, ctx->nmax_rows <= 256 ? 4 : 6);
        if (ctx->finish_strip) return smrt_launch::finish_strip(ctx, c);
        if (ctx->gmem_split) return smrt_launch::finish_gmem(ctx, c, grid, ctx->active);
        if (ctx->finish_strip4) return smrt_launch::finish_strip4(ctx, c);
        if (ctx->finish_reg) return smrt_launch::finish_reg(ctx, c);
        return ctx->active ? smrt_launch::active_finish(ctx, c, ctx->nt) : smrt_launch::finish(ctx, c, ctx->nt, ctx->finish2);
    };
    // lanes > 1: chunk k runs on lane stream k % lanes with the k % lanes-th region of the staging area (the launchers read
    // ctx->stream / ctx->stage, swapped for the duration of the chunk's launches; restored below)
    const hipStream_t main_stream = ctx->stream;
    const DevStage stage0 = ctx->stage;
    const int lanes = (ctx->lanes > 1 && d.pair_count > ctx->chunk_pairs) ? ctx->lanes : 1;
    struct Restore { smrt_dort_ctx* c; hipStream_t s; DevStage st; ~Restore() { c->stream = s; c->stage = st; } } restore{ctx, main_stream, stage0};
    if (lanes > 1) {
        hipError_t e;
        if ((e = hipEventRecord(ctx->fork_ev, main_stream)) != hipSuccess) return e;
        for (int k = 0; k < lanes; ++k)
            if ((e = hipStreamWaitEvent(ctx->lane_stream[k], ctx->fork_ev, 0)) != hipSuccess) return e;
    }
    // optional per-kernel timing: an event pair around every launch of a kind (on the stream the kernel goes to)
    auto timed = [&](int kind, auto&& launch) -> hipError_t {
        if (!ctx->breakdown_on) return launch();
        for (int k = 0; k < 2; ++k)
            if (ctx->bd_used + k >= ctx->bd_events.size()) {
                hipEvent_t ev;
                hipError_t e = hipEventCreate(&ev);
                if (e != hipSuccess) return e;
                ctx->bd_events.push_back(ev);
            }
        hipError_t e = hipEventRecord(ctx->bd_events[ctx->bd_used], ctx->stream);
        if (e != hipSuccess) return e;
        e = launch();
        if (e != hipSuccess) return e;
        e = hipEventRecord(ctx->bd_events[ctx->bd_used + 1], ctx->stream);
        ctx->bd_used += 2;
        ctx->bd_kind.push_back(kind);
        return e;
    };
    if (ctx->breakdown_on) { ctx->bd_used = 0; ctx->bd_kind.clear(); }
    long long chunk_index = 0;
    for (long long c0 = 0; c0 < d.pair_count; c0 += ctx->chunk_pairs, ++chunk_index) {
        const long long cn = std::min<long long>(ctx->chunk_pairs, d.pair_count - c0);
        DevBatch c = chunk_of(ctx, d, c0, cn);
        const unsigned grid = (unsigned)(ctx->gmem_path ? std::min<long long>(cn, ctx->gmem_grid) : cn);
        hipError_t e;
        const int lane = (int)(chunk_index % lanes);
        int* done_lane = (int*)ctx->d_done.p + (size_t)lane * ctx->chunk_pairs;
        if (lanes > 1) {
            const long long it0 = (long long)lane * ctx->chunk_pairs * items_per_pair;
            ctx->stream = ctx->lane_stream[lane];
            ctx->stage = stage0;
            ctx->stage.L = stage0.L + it0 * stage0.mat_stride; ctx->stage.B = stage0.B + it0 * stage0.mat_stride;
            ctx->stage.d = stage0.d + it0 * stage0.vec_stride; ctx->stage.sigma = stage0.sigma + it0 * stage0.vec_stride;
            ctx->stage.n = stage0.n + it0; ctx->stage.Linv = stage0.Linv + it0 * stage0.linv_stride;
            if (stage0.eig_rot) { ctx->stage.eig_e = stage0.eig_e + it0 * 2 * stage0.vec_stride; ctx->stage.eig_rot = stage0.eig_rot + it0 * stage0.rot_stride; }
            if (stage0.rec) ctx->stage.rec = stage0.rec + it0 * stage0.rec_stride;
            if (stage0.ws) ctx->stage.ws = stage0.ws + (long long)lane * ctx->chunk_pairs * rg::kSlotDoubles;
        }
        if (rounds > 1 || d.coherent) {   // unprocessed layers must read as "nothing staged", pairs as "not cut yet"
            if ((e = hipMemsetAsync(ctx->stage.n, 0, sizeof(int) * (size_t)(cn * items_per_pair), ctx->stream)) != hipSuccess) return e;
        }
        if (rounds > 1) {
            if ((e = hipMemsetAsync(done_lane, 0, sizeof(int) * (size_t)cn, ctx->stream)) != hipSuccess) return e;
            c.pair_done = (const int*)done_lane;
        }
        // the chunk's item lists for the launches per size class of rows; a round over part of the layers launches full grids
        ClassSegments segs{};
        const bool listed = ctx->class_lists && rounds == 1 && chunk_index < ctx->class_plan.chunks;
        for (int k = 0; listed && k < kRowClasses; ++k) {
            segs.list[k] = (const int*)ctx->d_cllist.p + ctx->class_plan.seg_offset[(size_t)chunk_index * kRowClasses + k];
            segs.count[k] = ctx->class_plan.seg_count[(size_t)chunk_index * kRowClasses + k];
        }
        const ClassSegments* seg = listed ? &segs : nullptr;
        for (int r = 0; r < rounds; ++r) {
            c.layer_lo = (int)((long long)d.Lmax * r / rounds);
            c.layer_hi = (int)((long long)d.Lmax * (r + 1) / rounds);
            if ((e = timed(0, [&]() { return prep(c, grid, seg); })) != hipSuccess) return e;
            const long long jitems = cn * modes * (c.layer_hi - c.layer_lo);
            if ((e = timed(1, [&]() { hipError_t e1 = ctx->big ? smrt_launch::jacobi_big(ctx, c, jitems) : ctx->eig ? smrt_launch::eig(ctx, c, jitems, seg) : smrt_launch::jacobi(ctx, c, jitems);
                                           if (e1 == hipSuccess && c.rayleigh_direct) e1 = smrt_launch::rayleigh(ctx, c, jitems);   // (its items leave the other kernels at once)
                                           return e1; })) != hipSuccess) return e;
            if (r + 1 < rounds && (e = smrt_launch::prune_mark(ctx, c, done_lane)) != hipSuccess) return e;
        }
        c.layer_lo = 0; c.layer_hi = d.Lmax; c.pair_done = nullptr;
        if ((e = timed(2, [&]() { return finish(c, grid); })) != hipSuccess) return e;
    }
    if (lanes > 1) {   // join: whatever follows on the context's stream (timing event, download, gather) waits for every lane
        for (int k = 0; k < lanes; ++k) {
            hipError_t e;
            if ((e = hipEventRecord(ctx->lane_ev[k], ctx->lane_stream[k])) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(main_stream, ctx->lane_ev[k], 0)) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

extern "C" {

const char* smrt_dort_version(void) { return "smrt_dort 0.1 (gfx950)"; }

int32_t smrt_dort_out_stride(const smrt_batch* b) { return smrt_host::out_stride(b); }

int32_t smrt_gauss_legendre_positive(int32_t n, double* mu, double* weight) {
    if (n < 1 || !mu) return -1;
    smrt_host::gauss_legendre_positive(n, mu, weight);
    return 0;
}

int32_t smrt_dort_device_count(void) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    return ndev;
}

int32_t smrt_dort_create(smrt_dort_ctx** out, int32_t device) {
    if (!out) return -1;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -2;  // no GPU: the product has no CPU fallback
    if (device < 0 || device >= ndev) return -3;
    smrt_dort_ctx* ctx = new smrt_dort_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
        delete ctx;
        return -4;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->max_lds = (int)prop.sharedMemPerBlock;
    if (ctx->max_lds < 160 * 1024) ctx->max_lds = 160 * 1024;  // gfx950: 160 KiB per workgroup
    *out = ctx;
    return 0;
}

void smrt_dort_destroy(smrt_dort_ctx* ctx) {
    if (!ctx) return;
    (void)smrt_dort_comm_destroy(ctx);
    (void)hipSetDevice(ctx->device);
    DevBuf* bufs[] = {&ctx->d_nl, &ctx->d_thick, &ctx->d_fv, &ctx->d_temp, &ctx->d_p1, &ctx->d_p2, &ctx->d_freq,
                      &ctx->d_theta, &ctx->d_gl, &ctx->d_out, &ctx->d_status, &ctx->d_layer, &ctx->d_stream, &ctx->d_n3, &ctx->d_stage, &ctx->d_work,
                      &ctx->d_stL, &ctx->d_stB, &ctx->d_std, &ctx->d_sts, &ctx->d_stn, &ctx->d_sti, &ctx->d_ste, &ctx->d_strot, &ctx->d_strec, &ctx->d_regws, &ctx->d_itfslot, &ctx->d_itf, &ctx->d_itfcoh,
                      &ctx->d_sub1, &ctx->d_sub2, &ctx->d_subT, &ctx->d_atm, &ctx->d_pairmap, &ctx->d_kind, &ctx->d_hostlayer, &ctx->d_hoststreams, &ctx->d_hostphase, &ctx->d_dispatch, &ctx->d_phase, &ctx->d_done, &ctx->d_lw, &ctx->d_clrows, &ctx->d_clcounts, &ctx->d_cloffsets, &ctx->d_cllist, &ctx->d_clmiss, &ctx->d_gather_out, &ctx->d_gather_status,
                      &ctx->d_scalar};
    for (DevBuf* b : bufs) b->release();
    smrt_launch::first_order_release(ctx);
    smrt_launch::successive_order_release(ctx);
    smrt_launch::successive_order_active_release(ctx);
    smrt_launch::multifresnel_release(ctx);
    smrt_launch::lrm_release(ctx);
    smrt_launch::sar_release(ctx);
    smrt_launch::second_order_release(ctx);
    smrt_launch::rough_release(ctx);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (int k = 0; k < 4; ++k) {
        if (ctx->lane_ev[k]) (void)hipEventDestroy(ctx->lane_ev[k]);
        if (ctx->lane_stream[k]) (void)hipStreamDestroy(ctx->lane_stream[k]);
    }
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    for (hipEvent_t ev : ctx->bd_events) (void)hipEventDestroy(ev);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* smrt_dort_last_error(const smrt_dort_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int32_t smrt_dort_set_pipeline(smrt_dort_ctx* ctx, int32_t split) {
    if (!ctx) return -1;
    ctx->split = (split != 0);
    ctx->finish2 = (split != 2);
    ctx->finish_mode = (split == 3) ? 1 : (split == 4 ? 0 : (split == 5 ? 2 : -1));   // 3: register-resident finish wherever supported, 4: no pivot-free kernel, 5: strip kernels wherever supported
    ctx->uploaded = false;  // the staging area is sized at upload time
    return 0;
}

int32_t smrt_dort_set_diagonalisation(smrt_dort_ctx* ctx, int32_t mode) {
    if (!ctx) return -1;
    if (mode < -1 || mode > SMRT_DIAG_SYMMETRIC) { ctx->err = "unknown diagonalisation mode"; return -1; }
    ctx->diag_mode = mode;
    ctx->uploaded = false;  // the staging area is sized at upload time
    return 0;
}

int32_t smrt_dort_set_prep(smrt_dort_ctx* ctx, int32_t mode) {
    if (!ctx) return -1;
    if (mode < -1 || mode > SMRT_PREP_PER_LAYER) { ctx->err = "unknown prep mode"; return -1; }
    ctx->prep_mode = mode;
    ctx->uploaded = false;  // the staging area is sized at upload time
    return 0;
}

int32_t smrt_dort_set_class_lists(smrt_dort_ctx* ctx, int32_t mode) {
    if (!ctx) return -1;
    if (mode < -1 || mode > 1) { ctx->err = "unknown class list mode"; return -1; }
    ctx->class_lists_mode = mode;
    ctx->uploaded = false;  // the lists are built at upload time
    return 0;
}

int32_t smrt_dort_finish_reg_lds_bytes(int32_t n_max_stream, int32_t n_layers_max) {
    return (int32_t)(sizeof(double) * (size_t)finish_reg_lds_doubles(n_max_stream, n_layers_max));
}

int32_t smrt_dort_finish_strip_lds_bytes(int32_t n_max_stream, int32_t n_layers_max, int32_t wavefronts) {
    if (wavefronts != 4 && wavefronts != 8) return -1;
    return (int32_t)(sizeof(double) * (size_t)finish_strip_lds_doubles(n_max_stream, n_layers_max, wavefronts));
}

int32_t smrt_dort_jacobi_lds_bytes(int32_t n_max_stream, int32_t n_pol, int32_t size_class_columns) {
    if (n_max_stream < 1 || (n_pol != 2 && n_pol != 3) || n_max_stream * n_pol > 128 || size_class_columns < 0) return -1;
    return (int32_t)(make_jacobi_plan(n_max_stream, n_pol, size_class_columns).total * sizeof(double));
}

int32_t smrt_dort_set_block_threads(smrt_dort_ctx* ctx, int32_t threads) {
    if (!ctx) return -1;
    if (threads == 0) threads = 256;
    if (threads != 64 && threads != 256) {   // one wavefront (the serial corner of every stage) or the tuned four
        ctx->err = "block threads must be 64 or 256";
        return -1;
    }
    ctx->nt = threads;
    return 0;
}

}  // extern "C"

// pairs == nullptr: the contiguous range [pair_begin, pair_begin + pair_count) of the flattened list; otherwise the
// n = pair_count listed pairs (pair_begin ignored)
static int32_t upload_impl(smrt_dort_ctx* ctx, const smrt_batch* b, int64_t pair_begin, int64_t pair_count,
                           const int64_t* pairs) {
    if (!ctx) return -1;
    const char* why = smrt_host::validate(b);
    if (why) { ctx->err = why; return -1; }
    // HIP's current device is per host thread: bind it BEFORE the first allocation below, or a buffer that has to
    // grow would land on whatever device the calling thread used last
    HIPCHK(hipSetDevice(ctx->device));
    ctx->active = (b->mode == SMRT_MODE_ACTIVE);
    if (ctx->active && (b->m_max < 0 || b->m_max > 64)) { ctx->err = "m_max must be in 0..64"; return -1; }
    const int64_t npairs = (int64_t)b->n_snowpacks * b->n_frequencies;
    if (pairs) {
        pair_begin = 0;
        if (pair_count <= 0) { ctx->err = "empty pair list"; return -1; }
        for (int64_t i = 0; i < pair_count; ++i)
            if (pairs[i] < 0 || pairs[i] >= npairs) { ctx->err = "pair index out of bounds"; return -1; }
    } else {
        if (pair_count < 0) pair_count = npairs - pair_begin;
        if (pair_begin < 0 || pair_count <= 0 || pair_begin + pair_count > npairs) { ctx->err = "pair range out of bounds"; return -1; }
    }
    const int P = ctx->active ? 3 : 2;
    const int nphi = ctx->active ? azimuth_samples(b->m_max) / 2 + 1 : 9;
    const int actd = ctx->active ? active_doubles(b->n_max_stream, b->n_layers_max, b->n_theta) : 0;
    const int actd_fin = ctx->active ? active_doubles(b->n_max_stream, b->n_layers_max, b->n_theta, false) : 0;   // finish kernels
    LdsPlan plan = make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, 1, actd);
    size_t lds = (size_t)plan.total * sizeof(double);
    ctx->gmem_path = (plan.NMAX > 64 || lds > (size_t)ctx->max_lds || getenv("SMRT_DORT_FORCE_GLOBAL_WORKSPACE") != nullptr);
    if (ctx->gmem_path) {
        if (plan.NMAX > 384) {
            ctx->err = "streams x polarisations above 384 (n_max_stream > 192 passive, > 128 active) is not supported by this build";
            return -1;
        }
        plan = make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, 0, actd, 0, 1);   // with an LDS Jacobi matrix
        ctx->jac_in_lds = 1;
        if ((size_t)plan.total * sizeof(double) > (size_t)ctx->max_lds) {
            plan = make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, 0, actd);
            ctx->jac_in_lds = 0;
        }
        lds = (size_t)plan.total * sizeof(double);
        if (lds > (size_t)ctx->max_lds) { ctx->err = "too many layers for the LDS-resident per-layer tables"; return -1; }
        ctx->gmem_grid = (int)std::min<int64_t>(pair_count, 1024);
        ctx->ws_stride = (long long)plan.mat_doubles + plan.scratch_doubles;
        HIPCHK(ctx->d_work.reserve(sizeof(double) * (size_t)ctx->gmem_grid * (size_t)ctx->ws_stride));
    }
    ctx->nmax_rows = plan.NMAX;
    ctx->chunk_pairs = 0;
    ctx->eig = false;
    // the per-layer prep (k_prep_layer.hip) in place of the per-pair prep kernel: the LDS pipelines in passive mode
    // (smrt_dort_set_prep / SMRT_DORT_PREP_LAYERS select; its item records count in the staging budget below)
    {
        int want = ctx->prep_mode < 0 ? SMRT_PREP_DEFAULT : ctx->prep_mode;
        if (const char* e = getenv("SMRT_DORT_PREP_LAYERS")) want = atoi(e) ? SMRT_PREP_PER_LAYER : SMRT_PREP_PER_PAIR;
        ctx->prep_layers = !ctx->gmem_path && ctx->split && !ctx->active && plan.NMAX <= 64 && want == SMRT_PREP_PER_LAYER;
    }
    const size_t rec_doubles = ctx->prep_layers ? (size_t)prep_record_doubles(b->n_max_stream) : 0;
    // the item lists of the launches per size class of rows (dort_class_lists.hpp): wanted unless switched off; whether this
    // batch has such launches is known below (ctx->eig)
    bool want_lists = ctx->class_lists_mode != 0;
    if (const char* e = getenv("SMRT_DORT_CLASS_LISTS")) want_lists = atoi(e) != 0;
    ctx->class_lists = false;
    ctx->class_plan.clear();
    // N > 128: the pipeline with the blocked Jacobi kernel (matrix in the staging area, column blocks through LDS)
    int big_min = 128;   // SMRT_DORT_BIG_MIN_N: experiments with the big pipeline on smaller matrices
    if (const char* e = getenv("SMRT_DORT_BIG_MIN_N")) big_min = std::max(64, atoi(e));
    ctx->big = ctx->gmem_path && ctx->split && plan.NMAX > big_min && getenv("SMRT_DORT_NO_BIG_PIPELINE") == nullptr &&
               (size_t)make_jacobi_big_plan(b->n_max_stream, P).total * sizeof(double) <= (size_t)ctx->max_lds;
    // 64 < N <= 128: the three-kernel pipeline needs the Jacobi kernel's own LDS matrix and the 16 N doubles of LDS scratch
    // of the finish kernel's blocked solvers -- NOT the whole-matrix Jacobi buffer of the fused kernel tested above (with 50
    // layers that plan misses the 160 KB by a few hundred bytes, and the batch must not fall back to the fused kernel,
    // four times slower, because of it)
    const bool split128 = ctx->gmem_path && ctx->split && !ctx->big && plan.NMAX <= 128 &&
        (size_t)make_jacobi_plan(b->n_max_stream, P).total * sizeof(double) <= (size_t)ctx->max_lds &&
        (size_t)make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, 0, actd_fin, 0, 2).total * sizeof(double) <= (size_t)ctx->max_lds &&
        (size_t)make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, 0, actd, 1).total * sizeof(double) <= (size_t)ctx->max_lds;
    if (split128) ctx->jac_in_lds = 1;   // what the kernels read as "the finish kernel has its LDS scratch"
    ctx->gmem_split = ctx->big || split128;
    if (ctx->big) ctx->jac_in_lds = 0;   // prep / finish of the big pipeline keep no Jacobi buffer in LDS
    if ((!ctx->gmem_path && ctx->split) || ctx->gmem_split) {
        const size_t nmodes = ctx->active ? (size_t)b->m_max + 1 : 1;   // staging items per layer
        const size_t mat = (size_t)plan.NMAX * plan.LD;
        const int linv_stride = (plan.NMAX > 64) ? 2048 : 1024;   // inverses of the diagonal blocks of L+: four or eight of 256 doubles
        const size_t per_pair = nmodes * b->n_layers_max * ((2 * mat + 2 * plan.NMAX + linv_stride + rec_doubles) * sizeof(double) + sizeof(int) +
                                                                  (want_lists && !ctx->active && plan.NMAX <= 64 ? 2 * sizeof(int) : 0));   // (rows and list entry of an item)
        // staging budget: 12 GB, or -- for the large matrices of the big pipeline, where 12 GB hold too few pairs to fill
        // the chip -- up to 60 % of the free device memory
        double budget = 12.0e9;
        if (ctx->big) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::max(budget, 0.6 * (double)(free_b + ctx->d_stL.cap + ctx->d_stB.cap));
        }
        // 64 < N <= 128: the finish kernels (and the Jacobi kernel) of this pipeline run ONE workgroup per CU, so a pass works in
        // rounds of 256 pairs and the 598 pairs that 12 GB hold at the configs[2] shape are 2.3 rounds (a third of the last one
        // idle): 40 GB and whole rounds
        const bool one_per_cu = ctx->gmem_split && !ctx->big;
        if (one_per_cu) budget = 40.0e9;
        long long chunk = (long long)(budget / (double)per_pair);
        if (chunk < 1) chunk = 1;
        if (one_per_cu && chunk >= 512) chunk -= chunk % 256;
        const long long chunk_cap = chunk;
        if (chunk > pair_count) chunk = pair_count;
        // the symmetric eigensolver in place of the Jacobi kernel (smrt_dort_set_diagonalisation): passive mode, N <= 64.
        // (Passive only: the backscatter is a small difference of intensities and needs the singular vectors of the small
        // singular values to the relative accuracy only the Jacobi iteration gives -- 3e-8 against 1e-8 relative on the
        // cross-polarised fixture of test_emulated_active_kernel_high_azimuth_order.)
        {
            int want = ctx->diag_mode < 0 ? SMRT_DIAG_SYMMETRIC : ctx->diag_mode;
            if (const char* e = getenv("SMRT_DORT_EIG")) want = atoi(e) ? SMRT_DIAG_SYMMETRIC : SMRT_DIAG_JACOBI;
            ctx->eig = !ctx->gmem_path && !ctx->active && plan.NMAX <= 64 && want == SMRT_DIAG_SYMMETRIC;
        }
        // (item indices in the lists are ints, local to a chunk)
        ctx->class_lists = want_lists && (ctx->prep_layers || ctx->eig) && chunk * (long long)b->n_layers_max < 0x7fffffffLL;
        ctx->lanes = 1;
        if (!ctx->gmem_path) {   // (the global-workspace pipelines share one per-workgroup workspace: one pass at a time)
            // With the eigensolver, three concurrent passes by default: its chase kernel is a latency chain of two wavefronts
            // per CU (64 KB of LDS each) that leaves the vector pipes to the tridiag / vectors kernels of the other passes --
            // 160 k -> 169 k solves/s on the headline batch (profiles/r6_eig_steps.txt); the Jacobi pipeline gains nothing
            // from it (round 4: profiles/r4_pipeline_lanes.txt)
            int want = ctx->eig ? 3 : SMRT_DORT_LANES_DEFAULT;
            if (const char* e = getenv("SMRT_DORT_LANES")) want = atoi(e);
            ctx->lanes = std::max(1, std::min(4, want));
            while (ctx->lanes > 1 && pair_count < 1024LL * ctx->lanes) --ctx->lanes;   // small batches: a pass should fill the chip
        }
        {   // equal chunks: a short last chunk would leave most of the chip idle for a whole pipeline pass
            long long nchunks = (pair_count + chunk - 1) / chunk;
            if (ctx->lanes > 1) nchunks = ((nchunks + ctx->lanes - 1) / ctx->lanes) * ctx->lanes;
            chunk = (pair_count + nchunks - 1) / nchunks;
            if (one_per_cu && nchunks > 1) chunk = std::min(chunk_cap, ((chunk + 255) / 256) * 256);   // whole rounds (the last chunk takes the rest)
        }
        ctx->chunk_pairs = chunk;
        for (int k = 0; k < ctx->lanes && ctx->lanes > 1; ++k) {
            if (!ctx->lane_stream[k]) HIPCHK(hipStreamCreateWithFlags(&ctx->lane_stream[k], hipStreamNonBlocking));
            if (!ctx->lane_ev[k]) HIPCHK(hipEventCreateWithFlags(&ctx->lane_ev[k], hipEventDisableTiming));
        }
        if (ctx->lanes > 1 && !ctx->fork_ev) HIPCHK(hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming));
        const size_t items = (size_t)chunk * ctx->lanes * b->n_layers_max * nmodes;
        HIPCHK(ctx->d_stL.reserve(items * mat * sizeof(double)));
        HIPCHK(ctx->d_stB.reserve(items * mat * sizeof(double)));
        HIPCHK(ctx->d_std.reserve(items * plan.NMAX * sizeof(double)));
        HIPCHK(ctx->d_sts.reserve(items * plan.NMAX * sizeof(double)));
        HIPCHK(ctx->d_stn.reserve(items * sizeof(int)));
        HIPCHK(ctx->d_sti.reserve(ctx->big ? 8 : items * linv_stride * sizeof(double)));   // (the N > 128 kernels do not stage them)
        ctx->stage.L = (double*)ctx->d_stL.p; ctx->stage.B = (double*)ctx->d_stB.p;
        ctx->stage.d = (double*)ctx->d_std.p; ctx->stage.sigma = (double*)ctx->d_sts.p;
        ctx->stage.n = (int*)ctx->d_stn.p; ctx->stage.Linv = ctx->big ? nullptr : (double*)ctx->d_sti.p;
        ctx->stage.linv_stride = linv_stride;
        ctx->stage.mat_stride = (long long)mat; ctx->stage.vec_stride = plan.NMAX;
        ctx->stage.rec = nullptr; ctx->stage.rec_stride = (int)rec_doubles;
        if (ctx->prep_layers) {
            HIPCHK(ctx->d_strec.reserve(items * rec_doubles * sizeof(double)));
            ctx->stage.rec = (double*)ctx->d_strec.p;
        }
        // the symmetric eigensolver in place of the Jacobi kernel (N <= 64: the LDS pipelines): its tridiagonal forms and
        // rotation lists (not counted in the staging budget above: 148 KB per item at N = 64 on top of the 67 KB of L+ and B)
        {
            ctx->stage.eig_e = nullptr; ctx->stage.eig_rot = nullptr; ctx->stage.rot_stride = 0;
            if (ctx->eig) {
                const long long rs = eig_rot_doubles(plan.NMAX);
                HIPCHK(ctx->d_ste.reserve(items * 2 * plan.NMAX * sizeof(double)));
                HIPCHK(ctx->d_strot.reserve(items * (size_t)rs * sizeof(double)));
                ctx->stage.eig_e = (double*)ctx->d_ste.p; ctx->stage.eig_rot = (double*)ctx->d_strot.p; ctx->stage.rot_stride = rs;
            }
        }
        ctx->jacobi_lds = ctx->big ? (size_t)make_jacobi_big_plan(b->n_max_stream, P).total * sizeof(double)
                                   : (size_t)make_jacobi_plan(b->n_max_stream, P).total * sizeof(double);
        ctx->jacobi16_lds = 0;
        if (ctx->gmem_split && !ctx->big) {
            const size_t l16 = (size_t)make_jacobi_plan(b->n_max_stream, P, 0, 16).total * sizeof(double);
            if (l16 <= (size_t)ctx->max_lds) ctx->jacobi16_lds = l16;
        }
        // (the LDS-resident passive prep kernel stores its two matrices as packed lower triangles: plan 3)
        ctx->prep_lds_bytes = (size_t)make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, ctx->gmem_split ? 0 : 1, actd,
                                                (!ctx->gmem_split && !ctx->active) ? 3 : 1).total * sizeof(double);
        ctx->finish2_lds_bytes = ctx->gmem_split
            ? (size_t)make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, 0, actd_fin, 0, ctx->big ? 3 : 2).total * sizeof(double)
            : (size_t)make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, 1, actd_fin, 2).total * sizeof(double);
    }
    // the register-resident finish kernel (one wavefront per pair, dort_finish_reg.hpp): LDS pipeline, passive mode, Flat
    // interfaces with T = 1 - R (no coherent slabs), no host-evaluated dense substrate
    {
        const bool supported = !ctx->gmem_path && ctx->split && ctx->finish2 && !ctx->active && ctx->chunk_pairs > 0 &&
                               !b->process_coherent_layers && b->substrate_kind != SUB_HOST && !b->host_interface_slot && !b->rough_kind;
        int want = (ctx->finish_mode == 2) ? -1 : ctx->finish_mode;
        if (const char* e = getenv("SMRT_DORT_FINISH_REG")) want = atoi(e) ? 1 : 0;
        ctx->finish_reg_lds_bytes = sizeof(double) * (size_t)finish_reg_lds_doubles(b->n_max_stream, b->n_layers_max);
        // (its per-layer tables grow with n_layers_max: beyond the LDS of a workgroup the two-slot kernel takes over)
        // NOT a default anywhere since round 5: the strip kernel on four wavefronts below takes every batch this kernel
        // supports while three of its workgroups share a CU (up to ~105 layers at 32 streams), and the per-layer tables of
        // the full LDS plan send a batch to the global-workspace pipeline from 92 layers on (32 streams) -- before that.
        // set_pipeline(3) / SMRT_DORT_FINISH_REG=1 select it (an independent second implementation of the pivot-free
        // recursion: the hard-input sweeps compare the two; tests/test_gpu_parity.py KERNEL_VARIANTS).
        const size_t cap = (want == 1) ? (size_t)64 * 1024 : (size_t)160 * 1024 / 3;
        ctx->finish_reg = supported && ctx->finish_reg_lds_bytes <= cap &&
                          (want == 1 || (want == -1 && SMRT_FINISH_REG_DEFAULT));
        ctx->stage.ws = nullptr;
        // The strip kernel's four-wavefront instance under the same conditions: the default while three of its workgroups
        // share a CU (160 KB / 3; 44 KB at 32 streams and 20 layers), with set_pipeline(5) up to the 64 KB a workgroup may
        // take; set_pipeline(3) keeps the register-resident kernel.  11.1 against 13.7 ms on the headline batch.
        ctx->finish_strip4 = false;
        {
            int want4 = (ctx->finish_mode == 2) ? 1 : (ctx->finish_mode == -1 ? -1 : 0);
            // (an explicit SMRT_DORT_FINISH_REG=1 asks for the register-resident kernel: it is not to lose against this
            // kernel's default -- ADVICE r5; SMRT_DORT_FINISH_STRIP4 still has the last word)
            if (getenv("SMRT_DORT_FINISH_REG") && want == 1 && want4 == -1) want4 = 0;
            if (const char* e = getenv("SMRT_DORT_FINISH_STRIP4")) want4 = atoi(e) ? 1 : 0;
            const size_t lds4 = sizeof(double) * (size_t)finish_strip_lds_doubles(b->n_max_stream, b->n_layers_max, 4);
            const size_t cap4 = (want4 == 1) ? (size_t)64 * 1024 : (size_t)160 * 1024 / 3;
            if (supported && lds4 <= cap4 && (want4 == 1 || (want4 == -1 && SMRT_FINISH_STRIP_DEFAULT))) {
                ctx->finish_strip4 = true; ctx->finish_strip4_lds_bytes = lds4; ctx->finish_reg = false;
                HIPCHK(ctx->d_regws.reserve(sizeof(double) * (size_t)ctx->chunk_pairs * ctx->lanes * StripFinish<4>::kWsDoubles));
                ctx->stage.ws = (double*)ctx->d_regws.p;
            }
        }
        if (ctx->finish_reg) {   // one 64 x 64 matrix per pair of a chunk in global memory (At between its two phases)
            HIPCHK(ctx->d_regws.reserve(sizeof(double) * (size_t)ctx->chunk_pairs * ctx->lanes * rg::kSlotDoubles));
            ctx->stage.ws = (double*)ctx->d_regws.p;
        }
    }
    // the strip finish kernel (one workgroup of eight wavefronts per pair, dort_finish_strip.hpp): the 64 < N <= 128 pipeline in
    // passive mode under the same conditions
    {
        const bool supported = ctx->gmem_split && !ctx->big && !ctx->active && plan.NMAX <= 128 && ctx->chunk_pairs > 0 &&
                               !b->process_coherent_layers && b->substrate_kind != SUB_HOST && !b->host_interface_slot && !b->rough_kind;
        int want = (ctx->finish_mode == 2) ? 1 : ctx->finish_mode;
        if (const char* e = getenv("SMRT_DORT_FINISH_STRIP")) want = atoi(e) ? 1 : 0;
        ctx->finish_strip_lds_bytes = sizeof(double) * (size_t)finish_strip_lds_doubles(b->n_max_stream, b->n_layers_max);
        ctx->finish_strip = supported && ctx->finish_strip_lds_bytes <= (size_t)ctx->max_lds &&
                            (want == 1 || (want == -1 && SMRT_FINISH_STRIP_DEFAULT));
        // ... and the LDS-resident prep kernel of the N <= 64 pipeline where its two packed triangles fit a CU's LDS
        ctx->prep_wide_lds_bytes = (size_t)make_plan(b->n_max_stream, P, b->n_layers_max, b->n_theta, nphi, 1, 0, 3).total * sizeof(double);
        ctx->prep_wide = ctx->gmem_split && !ctx->big && !ctx->active && plan.NMAX <= 128 && ctx->chunk_pairs > 0 &&
                         ctx->prep_wide_lds_bytes <= (size_t)ctx->max_lds && getenv("SMRT_DORT_NO_PREP_WIDE") == nullptr;
        if (ctx->finish_strip) {   // one 128 x 128 matrix per pair of a chunk in global memory (At between its two phases)
            HIPCHK(ctx->d_regws.reserve(sizeof(double) * (size_t)ctx->chunk_pairs * StripFinish<8>::kWsDoubles));
            ctx->stage.ws = (double*)ctx->d_regws.p;
        }
    }
    if (b->prune_optical_depth > 0.0) {
        // the kept layers are decided from the eigenvalues of ALL the layers before the bottom-up recursion starts:
        // only the three-kernel pipelines have them at that point
        const bool pipeline = ctx->chunk_pairs > 0 && (ctx->gmem_path || !ctx->active || ctx->finish2);
        if (!pipeline) {
            ctx->err = "prune_deep_snowpack needs the three-kernel pipeline (streams x polarisations <= 128, pipeline "
                       "1, or 2 in passive mode)";
            return -1;
        }
    }
    const size_t SL = (size_t)b->n_snowpacks * b->n_layers_max;
    if (upload_array(ctx, ctx->d_nl, b->n_layers, sizeof(int32_t) * b->n_snowpacks)) return -1;
    if (upload_array(ctx, ctx->d_thick, b->thickness, sizeof(double) * SL)) return -1;
    if (upload_array(ctx, ctx->d_fv, b->frac_volume, sizeof(double) * SL)) return -1;
    if (upload_array(ctx, ctx->d_temp, b->temperature, sizeof(double) * SL)) return -1;
    if (upload_array(ctx, ctx->d_p1, b->micro_p1, sizeof(double) * SL)) return -1;
    if (upload_array(ctx, ctx->d_p2, b->micro_p2 ? b->micro_p2 : b->micro_p1, sizeof(double) * SL)) return -1;
    if (upload_array(ctx, ctx->d_freq, b->frequency, sizeof(double) * b->n_frequencies)) return -1;
    if (upload_array(ctx, ctx->d_theta, b->theta, sizeof(double) * b->n_theta)) return -1;
    if (pairs && upload_array(ctx, ctx->d_pairmap, pairs, sizeof(int64_t) * pair_count)) return -1;
    if (b->layer_kind && upload_array(ctx, ctx->d_kind, b->layer_kind, sizeof(int32_t) * SL)) return -1;
    if (b->liquid_water && upload_array(ctx, ctx->d_lw, b->liquid_water, sizeof(double) * SL)) return -1;
    const size_t host_modes = ctx->active ? (size_t)b->m_max + 1 : 1, host_ne = (size_t)b->n_max_stream * P;
    if (b->host_layer) {   // scalars of the layers evaluated by the caller (SMRT_EM_HOST, SMRT_EM_IBA_HOST)
        const size_t PL = (size_t)npairs * b->n_layers_max;
        if (upload_array(ctx, ctx->d_hostlayer, b->host_layer, sizeof(double) * PL * 4)) return -1;
        if (b->host_iba_coeff && upload_array(ctx, ctx->d_hostcoeff, b->host_iba_coeff, sizeof(double) * PL)) return -1;
    }
    if (b->host_layer && b->host_streams && b->host_phase) {   // ... and their phase matrices (SMRT_EM_HOST)
        const size_t PL = (size_t)npairs * b->n_layers_max;
        if (upload_array(ctx, ctx->d_hoststreams, b->host_streams, sizeof(int32_t) * PL)) return -1;
        if (upload_array(ctx, ctx->d_hostphase, b->host_phase, sizeof(double) * PL * host_modes * 2 * host_ne * host_ne)) return -1;
    }
    const size_t FS = (size_t)b->n_snowpacks * b->n_frequencies;
    ctx->rough_info = {};
    if (b->host_interface_slot) {   // rough interfaces evaluated by the caller
        const size_t ne = 3 * (size_t)b->n_max_stream, nm = ctx->active ? (size_t)b->m_max + 1 : 1, ns = (size_t)b->host_interface_slots;
        if (upload_array(ctx, ctx->d_itfslot, b->host_interface_slot, sizeof(int32_t) * FS * b->n_layers_max)) return -1;
        if (upload_array(ctx, ctx->d_itf, b->host_interface, sizeof(double) * FS * ns * nm * 4 * ne * ne)) return -1;
        if (upload_array(ctx, ctx->d_itfcoh, b->host_interface_coh, sizeof(double) * FS * ns * 4 * ne)) return -1;
        ctx->rough_info.host_matrix_bytes += sizeof(double) * FS * ns * nm * 4 * ne * ne;
    }
    if (b->substrate_kind == SMRT_SUBSTRATE_HOST) {   // dense reflection matrices of a rough substrate, evaluated by the caller
        const size_t ne = 3 * (size_t)b->n_max_stream, nm = ctx->active ? (size_t)b->m_max + 1 : 1;
        if (upload_array(ctx, ctx->d_sub1, b->host_substrate, sizeof(double) * FS * nm * ne * ne)) return -1;
        if (upload_array(ctx, ctx->d_sub2, b->host_substrate_coh, sizeof(double) * FS * nm * ne)) return -1;
        if (b->substrate_temperature && upload_array(ctx, ctx->d_subT, b->substrate_temperature, sizeof(double) * b->n_snowpacks)) return -1;
        ctx->rough_info.host_matrix_bytes += sizeof(double) * FS * nm * ne * ne;
    } else
    if (smrt_host::rough_substrate(b)) {   // a rough substrate built on the device: its permittivity goes to the builder (rough_prepare)
        if (upload_array(ctx, ctx->d_subT, b->substrate_temperature, sizeof(double) * b->n_snowpacks)) return -1;
    } else
    if (b->substrate_kind != SMRT_SUBSTRATE_NONE) {
        const size_t sub_doubles = smrt_host::substrate_array_doubles(b);   // (the rough soils: + [S][2] parameters, smrt_dort.h)
        if (upload_array(ctx, ctx->d_sub1, b->substrate_p1, sizeof(double) * sub_doubles)) return -1;
        if (upload_array(ctx, ctx->d_sub2, b->substrate_p2, sizeof(double) * sub_doubles)) return -1;
        if (upload_array(ctx, ctx->d_subT, b->substrate_temperature, sizeof(double) * b->n_snowpacks)) return -1;
    }
    std::vector<double> atm;
    if (b->atm_tb_down) {
        atm.insert(atm.end(), b->atm_tb_down, b->atm_tb_down + b->n_frequencies);
        atm.insert(atm.end(), b->atm_tb_up, b->atm_tb_up + b->n_frequencies);
        atm.insert(atm.end(), b->atm_transmittance, b->atm_transmittance + b->n_frequencies);
        if (upload_array(ctx, ctx->d_atm, atm.data(), sizeof(double) * atm.size())) return -1;
    }
    std::vector<double> gl(b->n_max_stream);
    smrt_host::gauss_legendre_positive(b->n_max_stream, gl.data(), nullptr);
    if (upload_array(ctx, ctx->d_gl, gl.data(), sizeof(double) * gl.size())) return -1;
    ctx->out_stride = smrt_host::out_stride(b);
    HIPCHK(ctx->d_out.reserve(sizeof(double) * pair_count * ctx->out_stride));
    HIPCHK(ctx->d_status.reserve(sizeof(int32_t) * pair_count));
    HIPCHK(ctx->d_layer.reserve(sizeof(double) * pair_count * b->n_layers_max * 5));
    HIPCHK(ctx->d_stream.reserve(sizeof(double) * pair_count * (1 + b->n_max_stream)));
    HIPCHK(ctx->d_n3.reserve(sizeof(double) * pair_count));
    HIPCHK(ctx->d_stage.reserve(sizeof(double) * pair_count * 16));
    HIPCHK(hipMemsetAsync(ctx->d_stage.p, 0, sizeof(double) * pair_count * 16, ctx->stream));
    DevBatch& d = ctx->dev;
    d.S = b->n_snowpacks; d.Lmax = b->n_layers_max; d.F = b->n_frequencies; d.n_theta = b->n_theta;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.mode = b->mode; d.n_max_stream = b->n_max_stream;
    d.m_max = b->m_max; d.normalization = b->phase_normalization; d.rayleigh_jeans = b->rayleigh_jeans;
    d.want_layer_out = 1; d.want_stream_out = 1;
    d.jac_in_lds = ctx->gmem_path ? ctx->jac_in_lds : 0;
    d.pair_begin = pair_begin; d.pair_count = pair_count;
    d.pair_map = pairs ? (const long long*)ctx->d_pairmap.p : nullptr;
    d.n_layers = (const int*)ctx->d_nl.p; d.thickness = (const double*)ctx->d_thick.p;
    d.frac_volume = (const double*)ctx->d_fv.p; d.temperature = (const double*)ctx->d_temp.p;
    d.p1 = (const double*)ctx->d_p1.p; d.p2 = (const double*)ctx->d_p2.p;
    d.frequency = (const double*)ctx->d_freq.p; d.theta = (const double*)ctx->d_theta.p;
    d.gl_mu = (const double*)ctx->d_gl.p; d.phi = b->phi;
    d.layer_kind = b->layer_kind ? (const int*)ctx->d_kind.p : nullptr;
    d.liquid_water = b->liquid_water ? (const double*)ctx->d_lw.p : nullptr;
    const bool has_host = b->host_layer && b->host_streams && b->host_phase;
    d.host_layer = b->host_layer ? (const double*)ctx->d_hostlayer.p : nullptr;
    d.host_coeff = (b->host_layer && b->host_iba_coeff) ? (const double*)ctx->d_hostcoeff.p : nullptr;
    d.host_streams = has_host ? (const int*)ctx->d_hoststreams.p : nullptr;
    d.host_phase = has_host ? (const double*)ctx->d_hostphase.p : nullptr;
    d.host_modes = (int)host_modes; d.host_ne = (int)host_ne;
    d.coherent = b->process_coherent_layers ? 1 : 0;
    d.sub_kind = b->substrate_kind;
    d.sub_p1 = (const double*)ctx->d_sub1.p; d.sub_p2 = (const double*)ctx->d_sub2.p; d.sub_T = (const double*)ctx->d_subT.p;
    d.host_itf_slot = b->host_interface_slot ? (const int*)ctx->d_itfslot.p : nullptr;
    d.host_itf = b->host_interface_slot ? (const double*)ctx->d_itf.p : nullptr;
    d.host_itf_coh = b->host_interface_slot ? (const double*)ctx->d_itfcoh.p : nullptr;
    d.host_itf_slots = b->host_interface_slot ? b->host_interface_slots : 0;
    d.host_substrate = (const double*)ctx->d_sub1.p; d.host_substrate_coh = (const double*)ctx->d_sub2.p;   // (SUB_HOST: the same buffers)
    const bool has_atm = (b->atm_tb_down != nullptr) && b->mode == SMRT_MODE_PASSIVE;
    d.atm_down = has_atm ? (const double*)ctx->d_atm.p : nullptr;
    d.atm_up = has_atm ? (const double*)ctx->d_atm.p + b->n_frequencies : nullptr;
    d.atm_trans = has_atm ? (const double*)ctx->d_atm.p + 2 * b->n_frequencies : nullptr;
    d.prune_tau = (b->prune_optical_depth > 0.0) ? b->prune_optical_depth : 0.0;
    d.layer_lo = 0; d.layer_hi = b->n_layers_max; d.pair_done = nullptr;
    d.class_list = nullptr; d.class_miss = nullptr;
    if (d.prune_tau > 0.0) HIPCHK(ctx->d_done.reserve(sizeof(int) * (size_t)std::max<long long>(ctx->chunk_pairs, 1) * ctx->lanes));
    // Jacobi thresholds on the squared cosine between two columns: below skip2 a pair is not rotated, a sweep without
    // a rotation above exit2 is the last one (dort_jacobi_kernel.hpp).  SMRT_DORT_JACOBI_SKIP2 / _EXIT2 override them
    // for experiments.  Passive mode, measured on the headline batch against the oracle (profiles/r3_jacobi_thresholds.txt):
    // 1e-26 / 1e-15 -> 1.4e-10 K, 1e-22 / 1e-12 -> 1.6e-8 K (2.6 % faster), 1e-20 / 1e-10 -> 2.4e-7 K; the requirement is 1e-6 K.
    // The register-resident finish kernel needs the tighter pair on weakly scattering media (dort_host_common.hpp).
    const bool orth = ctx->finish_reg || ctx->finish_strip || ctx->finish_strip4;   // the finish kernels that use the orthogonality of B' itself
    d.jacobi_skip2 = ctx->active ? 1e-30 : (orth ? SMRT_JACOBI_REG_SKIP_COS2 : SMRT_JACOBI_PASSIVE_SKIP_COS2);
    d.jacobi_exit2 = ctx->active ? 1e-22 : (orth ? SMRT_JACOBI_REG_EXIT_COS2 : SMRT_JACOBI_PASSIVE_EXIT_COS2);
    if (const char* e = getenv("SMRT_DORT_JACOBI_SKIP2")) d.jacobi_skip2 = atof(e);
    if (const char* e = getenv("SMRT_DORT_JACOBI_EXIT2")) d.jacobi_exit2 = atof(e);
    d.out = (double*)ctx->d_out.p; d.status = (int*)ctx->d_status.p; d.layer_out = (double*)ctx->d_layer.p;
    d.stream_out = (double*)ctx->d_stream.p; d.n3_out = (double*)ctx->d_n3.p; d.stage_out = (double*)ctx->d_stage.p;
    // Layers with a Rayleigh phase matrix in closed form (dort_rayleigh_kernel.hpp) wherever a strip finish kernel reads the
    // staging area -- it takes A+ = D V as it is -- and the batch can hold such layers; SMRT_DORT_RAYLEIGH=0: the Cholesky +
    // Jacobi route for them too (A/B switch)
    {
        const bool may_hold = b->layer_kind != nullptr || em_has_rayleigh_phase(b->emmodel);
        const char* e = getenv("SMRT_DORT_RAYLEIGH");
        d.rayleigh_direct = (!ctx->active && (ctx->finish_strip || ctx->finish_strip4) && ctx->stage.Linv && may_hold && !(e && atoi(e) == 0)) ? 1 : 0;
    }
    ctx->lds_bytes = lds;
    if (b->rough_kind && smrt_launch::rough_prepare(ctx, b, d)) return -1;
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the staging vector `gl` and the caller's arrays may go away
    ctx->uploaded = true;
    // Dispatch order: inside every chunk the workgroups take the pairs sorted by their estimated cost (sum of N_l^3 from the
    // stream counts: a cheap kernel).  Neighbouring workgroups -- the ones that share a CU -- then work on matrices of the
    // same size: 59.9 instead of 61.4 ms on the headline batch, whichever way the sort goes (tools/lpt_order_probe.py).
    // The outputs stay in the caller's order (only the workgroup -> pair map changes).  SMRT_DORT_NO_COST_ORDER=1: off.
    // The same kernel counts, per pair, its items in every size class of rows; the counts come back with the costs, and once
    // the dispatch order is known the lists are laid out (host) and filled (device, on the stream: before any launch).
    d.dispatch = nullptr;
    const bool cost_order = pair_count > 1 && getenv("SMRT_DORT_NO_COST_ORDER") == nullptr;
    if (cost_order || ctx->class_lists) {
        const long long Lmax = b->n_layers_max;
        int *rows_dev = nullptr, *counts_dev = nullptr;
        if (ctx->class_lists) {
            HIPCHK(ctx->d_clrows.reserve(sizeof(int) * (size_t)(pair_count * Lmax)));
            HIPCHK(ctx->d_clcounts.reserve(sizeof(int) * (size_t)pair_count * kRowClasses));
            HIPCHK(ctx->d_clmiss.reserve(sizeof(unsigned long long)));
            HIPCHK(hipMemsetAsync(ctx->d_clmiss.p, 0, sizeof(unsigned long long), ctx->stream));
            rows_dev = (int*)ctx->d_clrows.p; counts_dev = (int*)ctx->d_clcounts.p;
            d.class_miss = (unsigned long long*)ctx->d_clmiss.p;
        }
        HIPCHK(smrt_launch::pair_cost(ctx, d, d.n3_out, rows_dev, counts_dev));
        std::vector<double> cost((size_t)pair_count);
        HIPCHK(hipMemcpyAsync(cost.data(), d.n3_out, sizeof(double) * cost.size(), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->class_lists) {
            ctx->class_counts_host.resize((size_t)pair_count * kRowClasses);
            HIPCHK(hipMemcpyAsync(ctx->class_counts_host.data(), counts_dev, sizeof(int32_t) * ctx->class_counts_host.size(), hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        const long long chunk = ctx->chunk_pairs > 0 ? ctx->chunk_pairs : pair_count;
        if (cost_order) {
            std::vector<int32_t>& order = ctx->dispatch_host;
            order.resize((size_t)pair_count);
            for (long long c0 = 0; c0 < pair_count; c0 += chunk) {
                const long long cn = std::min<long long>(chunk, pair_count - c0);
                for (long long i = 0; i < cn; ++i) order[(size_t)(c0 + i)] = (int32_t)i;    // chunk-local pair slots
                std::stable_sort(order.begin() + c0, order.begin() + c0 + cn,
                                 [&](int32_t a, int32_t b2) { return cost[(size_t)(c0 + a)] > cost[(size_t)(c0 + b2)]; });
            }
            if (upload_array(ctx, ctx->d_dispatch, order.data(), sizeof(int32_t) * order.size())) return -1;
            d.dispatch = (const int*)ctx->d_dispatch.p;
        }
        if (ctx->class_lists) {
            ctx->class_plan = make_class_list_plan(ctx->class_counts_host.data(), cost_order ? ctx->dispatch_host.data() : nullptr, pair_count, chunk);
            if (upload_array(ctx, ctx->d_cloffsets, ctx->class_plan.pair_offset.data(), sizeof(long long) * ctx->class_plan.pair_offset.size())) return -1;
            HIPCHK(ctx->d_cllist.reserve(sizeof(int) * (size_t)std::max<long long>(ctx->class_plan.total, 1)));
            HIPCHK(smrt_launch::class_fill(ctx, d, chunk, rows_dev, (const long long*)ctx->d_cloffsets.p, (int*)ctx->d_cllist.p));
        }
    }
    return 0;
}

extern "C" {

int32_t smrt_dort_upload(smrt_dort_ctx* ctx, const smrt_batch* b, int64_t pair_begin, int64_t pair_count) {
    return upload_impl(ctx, b, pair_begin, pair_count, nullptr);
}

int32_t smrt_dort_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* b, const int64_t* pairs, int64_t n_pairs) {
    if (ctx && !pairs) { ctx->err = "null pair list"; return -1; }
    return upload_impl(ctx, b, 0, n_pairs, pairs);
}

int32_t smrt_dort_abi(int32_t* out, int32_t capacity) {
#define SMRT_OFF(f) (int32_t)offsetof(smrt_batch, f)
    const int32_t desc[] = {(int32_t)sizeof(smrt_batch),
        SMRT_OFF(n_snowpacks), SMRT_OFF(n_layers_max), SMRT_OFF(n_frequencies), SMRT_OFF(n_theta), SMRT_OFF(emmodel),
        SMRT_OFF(microstructure), SMRT_OFF(mode), SMRT_OFF(n_max_stream), SMRT_OFF(m_max), SMRT_OFF(phase_normalization),
        SMRT_OFF(rayleigh_jeans), SMRT_OFF(substrate_kind), SMRT_OFF(n_layers), SMRT_OFF(thickness), SMRT_OFF(frac_volume),
        SMRT_OFF(temperature), SMRT_OFF(micro_p1), SMRT_OFF(micro_p2), SMRT_OFF(frequency), SMRT_OFF(theta), SMRT_OFF(phi),
        SMRT_OFF(substrate_p1), SMRT_OFF(substrate_p2), SMRT_OFF(substrate_temperature), SMRT_OFF(atm_tb_down),
        SMRT_OFF(atm_tb_up), SMRT_OFF(atm_transmittance), SMRT_OFF(prune_optical_depth), SMRT_OFF(layer_kind),
        SMRT_OFF(host_layer), SMRT_OFF(host_streams), SMRT_OFF(host_phase), SMRT_OFF(process_coherent_layers),
        SMRT_OFF(host_substrate), SMRT_OFF(host_substrate_coh), SMRT_OFF(host_interface_slot), SMRT_OFF(host_interface),
        SMRT_OFF(host_interface_coh), SMRT_OFF(host_interface_slots), SMRT_OFF(liquid_water), SMRT_OFF(host_iba_coeff),
        SMRT_OFF(rough_kind), SMRT_OFF(rough_params)};
#undef SMRT_OFF
    const int32_t n = (int32_t)(sizeof(desc) / sizeof(desc[0]));
    for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = desc[i];
    return n;
}

int32_t smrt_dort_rough_matrices(smrt_dort_ctx* ctx, const smrt_batch* b, int32_t* slot, double* itf, double* itf_coh, double* sub,
                                 double* sub_coh) {
    if (!ctx) return -1;
    if (!b || !b->rough_kind) { ctx->err = "smrt_dort_rough_matrices needs a batch with rough_kind"; return -1; }
    if (upload_impl(ctx, b, 0, -1, nullptr)) return -1;
    const size_t FS = (size_t)b->n_snowpacks * b->n_frequencies, ne = 3 * (size_t)b->n_max_stream, nm = ctx->active ? (size_t)b->m_max + 1 : 1;
    const size_t ns = (size_t)ctx->rough_info.slots;
    if (ns > 0) {
        if (slot) HIPCHK(hipMemcpy(slot, ctx->d_itfslot.p, sizeof(int32_t) * FS * b->n_layers_max, hipMemcpyDeviceToHost));
        if (itf) HIPCHK(hipMemcpy(itf, ctx->d_itf.p, sizeof(double) * FS * ns * nm * 4 * ne * ne, hipMemcpyDeviceToHost));
        if (itf_coh) HIPCHK(hipMemcpy(itf_coh, ctx->d_itfcoh.p, sizeof(double) * FS * ns * 4 * ne, hipMemcpyDeviceToHost));
    }
    if (ctx->rough_info.has_sub) {
        if (sub) HIPCHK(hipMemcpy(sub, ctx->d_sub1.p, sizeof(double) * FS * nm * ne * ne, hipMemcpyDeviceToHost));
        if (sub_coh) HIPCHK(hipMemcpy(sub_coh, ctx->d_sub2.p, sizeof(double) * FS * nm * ne, hipMemcpyDeviceToHost));
    }
    return (int32_t)ns;
}

int32_t smrt_dort_rough_info(smrt_dort_ctx* ctx, double* info, int32_t n) {
    if (!ctx || !info || n < 0) return -1;
    // [5]: bytes the builder may take for its matrices -- what it holds already plus the device's free memory
    size_t free_b = 0, total_b = 0;
    if (n > 5 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    const double v[6] = {(double)SMRT_ROUGH_M_MAX, (double)ctx->rough_info.slots, (double)ctx->rough_info.ms,
                         (double)ctx->rough_info.built_bytes, (double)ctx->rough_info.host_matrix_bytes,
                         (double)(free_b + ctx->d_itf.cap + ctx->d_sub1.cap)};
    for (int k = 0; k < n && k < 6; ++k) info[k] = v[k];
    return 6;
}

int32_t smrt_dort_launch(smrt_dort_ctx* ctx, void* out_dev, void* status_dev) {
    if (!ctx) return -1;
    if (!ctx->uploaded) { ctx->err = "no batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    DevBatch d = ctx->dev;
    if (out_dev) d.out = (double*)out_dev;
    if (status_dev) d.status = (int*)status_dev;
    if (ctx->timing_pending) {  // fold the previous launch into the totals before reusing the events
        HIPCHK(hipEventSynchronize(ctx->ev1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->last_ms = ms; ctx->total_ms += ms; ctx->n_launch++;
        ctx->timing_pending = false;
    }
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    hipError_t e;
    const bool lds_pipeline = !ctx->gmem_path && ctx->split && ctx->chunk_pairs > 0 && (!ctx->active || ctx->finish2);
    if (ctx->gmem_split || lds_pipeline) e = launch_pipeline(ctx, d);
    else if (ctx->gmem_path) e = smrt_launch::fused_gmem(ctx, d, ctx->nmax_rows <= 128 ? 2 : ctx->nmax_rows <= 256 ? 4 : 6, ctx->active);
    else e = smrt_launch::fused(ctx, d, ctx->nt, ctx->active);
    HIPCHK(e);
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timing_pending = true;
    return 0;
}

int32_t smrt_dort_sync(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->timing_pending) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->last_ms = ms; ctx->total_ms += ms; ctx->n_launch++;
        ctx->timing_pending = false;
    }
    return 0;
}

double smrt_dort_last_kernel_ms(smrt_dort_ctx* ctx) { return ctx ? (double)ctx->last_ms : -1.0; }

int32_t smrt_dort_kernel_breakdown(smrt_dort_ctx* ctx, int32_t enable, double* ms3) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    if (ms3) {   // the intervals recorded by the last launch, summed per kind (synchronises)
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ms3[0] = ms3[1] = ms3[2] = 0.0;
        for (size_t k = 0; k < ctx->bd_kind.size() && 2 * k + 1 < ctx->bd_used; ++k) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ctx->bd_events[2 * k], ctx->bd_events[2 * k + 1]));
            ms3[ctx->bd_kind[k]] += ms;
        }
    }
    const int32_t recorded = (int32_t)ctx->bd_kind.size();
    if (enable >= 0) {   // (negative: read only, the instrumentation stays as it is)
        ctx->breakdown_on = (enable != 0);
        if (!ctx->breakdown_on) { ctx->bd_used = 0; ctx->bd_kind.clear(); }
    }
    return recorded;
}

int32_t smrt_dort_launch_info(smrt_dort_ctx* ctx, int64_t* info, int32_t n) {
    if (!ctx || !info || n < 0) return -1;
    if (!ctx->uploaded) { ctx->err = "no batch uploaded"; return -1; }
    const DevBatch& d = ctx->dev;
    const bool lds_pipeline = !ctx->gmem_path && ctx->split && ctx->chunk_pairs > 0 && (!ctx->active || ctx->finish2);
    int64_t v[SMRT_INFO_COUNT] = {0};
    v[SMRT_INFO_PIPELINE] = ctx->gmem_split ? (ctx->big ? SMRT_PIPELINE_BIG : ctx->finish_strip ? SMRT_PIPELINE_GMEM_STRIP : SMRT_PIPELINE_GMEM)
                          : lds_pipeline ? (ctx->finish_strip4 ? SMRT_PIPELINE_LDS_STRIP : ctx->finish_reg ? SMRT_PIPELINE_LDS_REG : ctx->finish2 ? SMRT_PIPELINE_LDS_TWO_SLOT : SMRT_PIPELINE_LDS_FOUR_SLOT)
                          : ctx->gmem_path ? SMRT_PIPELINE_FUSED_GMEM : SMRT_PIPELINE_FUSED;
    const bool three = ctx->gmem_split || lds_pipeline;
    v[SMRT_INFO_CHUNK_PAIRS] = three ? ctx->chunk_pairs : d.pair_count;
    v[SMRT_INFO_CHUNKS] = three ? (d.pair_count + ctx->chunk_pairs - 1) / ctx->chunk_pairs : 1;
    const int rounds = (three && d.prune_tau > 0.0 && !d.coherent && getenv("SMRT_DORT_NO_PRUNE_ROUNDS") == nullptr) ? std::min(4, d.Lmax) : 1;
    v[SMRT_INFO_PRUNE_ROUNDS] = rounds;
    v[SMRT_INFO_STAGED_ITEMS] = -1;
    if (three && (rounds > 1 || d.coherent) && ctx->n_launch + (ctx->timing_pending ? 1 : 0) > 0) {
        // the staging counts of the LAST chunk of the last launch (reset before every chunk in these modes): how many
        // (pair, mode, layer) items were diagonalised -- under prune_deep_snowpack the layers below a cut are not
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        const long long items_per_pair = (long long)(ctx->active ? d.m_max + 1 : 1) * d.Lmax;
        const long long last = d.pair_count - (v[SMRT_INFO_CHUNKS] - 1) * ctx->chunk_pairs;
        std::vector<int> h((size_t)(last * items_per_pair));
        const int lanes = (ctx->lanes > 1 && d.pair_count > ctx->chunk_pairs) ? ctx->lanes : 1;
        const long long lane = (v[SMRT_INFO_CHUNKS] - 1) % lanes;    // the staging region the last chunk ran in
        HIPCHK(hipMemcpy(h.data(), ctx->stage.n + lane * ctx->chunk_pairs * items_per_pair, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
        long long staged = 0;
        for (int x : h) staged += (x > 0);
        v[SMRT_INFO_STAGED_ITEMS] = staged;
    }
    v[SMRT_INFO_BLOCK_THREADS] = ctx->nt;
    v[SMRT_INFO_N_MAX] = ctx->nmax_rows;
    v[SMRT_INFO_DIAGONALISATION] = (three && ctx->eig) ? SMRT_DIAG_SYMMETRIC : SMRT_DIAG_JACOBI;
    v[SMRT_INFO_RAYLEIGH_CLOSED_FORM] = (three && d.rayleigh_direct) ? 1 : 0;
    v[SMRT_INFO_PREP] = (lds_pipeline && ctx->prep_layers) ? SMRT_PREP_PER_LAYER : SMRT_PREP_PER_PAIR;
    // (lists are built per upload; a launch in prune rounds still runs full grids)
    v[SMRT_INFO_CLASS_LISTS] = (lds_pipeline && ctx->class_lists && rounds == 1) ? 1 : 0;
    v[SMRT_INFO_CLASS_LIST_ITEMS] = (lds_pipeline && ctx->class_lists) ? ctx->class_plan.total : -1;
    v[SMRT_INFO_CLASS_LIST_MISSES] = 0;
    if (lds_pipeline && ctx->class_lists) {   // synchronises
        unsigned long long misses = 0;
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(&misses, ctx->d_clmiss.p, sizeof(misses), hipMemcpyDeviceToHost));
        v[SMRT_INFO_CLASS_LIST_MISSES] = (int64_t)misses;
    }
    for (int k = 0; k < n && k < SMRT_INFO_COUNT; ++k) info[k] = v[k];
    return SMRT_INFO_COUNT;
}

double smrt_dort_total_kernel_ms(smrt_dort_ctx* ctx, int64_t* n_launches, int32_t reset) {
    if (!ctx) return -1.0;
    const double tot = ctx->total_ms;
    if (n_launches) *n_launches = ctx->n_launch;
    if (reset) { ctx->total_ms = 0.0; ctx->n_launch = 0; }
    return tot;
}

int32_t smrt_dort_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* stream_out) {
    if (!ctx) return -1;
    if (!ctx->uploaded) { ctx->err = "no batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const DevBatch& d = ctx->dev;
    const size_t np = (size_t)d.pair_count;
    if (out) HIPCHK(hipMemcpyAsync(out, d.out, sizeof(double) * np * ctx->out_stride, hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d.status, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream));
    if (layer_out) HIPCHK(hipMemcpyAsync(layer_out, d.layer_out, sizeof(double) * np * d.Lmax * 5, hipMemcpyDeviceToHost, ctx->stream));
    if (stream_out) HIPCHK(hipMemcpyAsync(stream_out, d.stream_out, sizeof(double) * np * (1 + d.n_max_stream), hipMemcpyDeviceToHost, ctx->stream));
    return smrt_dort_sync(ctx);
}

double smrt_dort_sum_n3(smrt_dort_ctx* ctx) {
    if (!ctx || !ctx->uploaded) return -1.0;
    if (hipSetDevice(ctx->device) != hipSuccess) return -1.0;
    std::vector<double> h((size_t)ctx->dev.pair_count);
    if (hipMemcpy(h.data(), ctx->dev.n3_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
    double s = 0.0;
    for (double v : h) s += v;
    return s;
}

int32_t smrt_dort_ft_even_phase(smrt_dort_ctx* ctx, int32_t emmodel, int32_t microstructure, double frequency, double frac_volume,
                                double temperature, double micro_p1, double micro_p2, const double* mu_s, int32_t n_s,
                                const double* mu_i, int32_t n_i, int32_t m_max, int32_t npol, double* out) {
    if (!ctx) return -1;
    if (!mu_s || !mu_i || !out || n_s < 1 || n_i < 1 || m_max < 0 || m_max > 64 || (npol != 2 && npol != 3)) {
        ctx->err = "invalid ft_even_phase request";
        return -1;
    }
    if (emmodel < SMRT_EM_IBA || (emmodel > SMRT_EM_NONSCATTERING && emmodel != SMRT_EM_IBA_INVERTED) ||
        (microstructure != SMRT_MS_EXPONENTIAL && microstructure != SMRT_MS_STICKY_HARD_SPHERES)) {
        ctx->err = "unknown emmodel / microstructure";
        return -1;
    }
    for (int i = 0; i < n_s; ++i) if (!(fabs(mu_s[i]) <= 1.0)) { ctx->err = "cosines must lie in [-1, 1]"; return -1; }
    for (int i = 0; i < n_i; ++i) if (!(fabs(mu_i[i]) <= 1.0)) { ctx->err = "cosines must lie in [-1, 1]"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n_out = (size_t)npol * npol * (m_max + 1) * n_s * n_i;
    const size_t bytes = sizeof(double) * (n_out + n_s + n_i) + 16;
    HIPCHK(ctx->d_phase.reserve(bytes));
    double* d_out = (double*)ctx->d_phase.p;
    double* d_mus = d_out + n_out;
    double* d_mui = d_mus + n_s;
    int* d_status = (int*)(d_mui + n_i);
    HIPCHK(hipMemcpyAsync(d_mus, mu_s, sizeof(double) * n_s, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_mui, mu_i, sizeof(double) * n_i, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(d_status, 0, sizeof(int), ctx->stream));
    PhaseRequest q{emmodel, microstructure, frequency, frac_volume, temperature, micro_p1, micro_p2, d_mus, n_s, d_mui, n_i,
                   m_max, npol, azimuth_samples(m_max), d_out, d_status};
    HIPCHK(smrt_launch::ft_even_phase(ctx, q));
    int st = 0;
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&st, d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (st != 0) { ctx->err = "invalid layer properties (temperature above the freezing point?)"; return -1; }
    return 0;
}

int32_t smrt_dort_pair_cost(smrt_dort_ctx* ctx, double* cost) {
    if (!ctx || !cost) return -1;
    if (!ctx->uploaded) { ctx->err = "no batch uploaded"; return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    // the work counter buffer of the solve doubles as the output (a launch overwrites it anyway)
    HIPCHK(smrt_launch::pair_cost(ctx, ctx->dev, ctx->dev.n3_out));
    HIPCHK(hipMemcpyAsync(cost, ctx->dev.n3_out, sizeof(double) * (size_t)ctx->dev.pair_count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int32_t smrt_dort_stage_cycles(smrt_dort_ctx* ctx, double* out16) {
    if (!ctx || !ctx->uploaded || !out16) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<double> h((size_t)ctx->dev.pair_count * 16);
    HIPCHK(hipMemcpy(h.data(), ctx->dev.stage_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) out16[k] = 0.0;
    for (size_t p = 0; p < (size_t)ctx->dev.pair_count; ++p)
        for (int k = 0; k < 16; ++k) out16[k] += h[p * 16 + k];
    return 0;
}

int32_t smrt_dort_run(smrt_dort_ctx* ctx, const smrt_batch* batch, int64_t pair_begin, int64_t pair_count, double* out,
                      int32_t* status, double* layer_out, double* stream_out) {
    if (smrt_dort_upload(ctx, batch, pair_begin, pair_count)) return -1;
    if (smrt_dort_launch(ctx, nullptr, nullptr)) return -1;
    return smrt_dort_download(ctx, out, status, layer_out, stream_out);
}

int32_t smrt_dort_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const int64_t* pairs, int64_t n_pairs, double* out,
                            int32_t* status, double* layer_out, double* stream_out) {
    if (smrt_dort_upload_pairs(ctx, batch, pairs, n_pairs)) return -1;
    if (smrt_dort_launch(ctx, nullptr, nullptr)) return -1;
    return smrt_dort_download(ctx, out, status, layer_out, stream_out);
}

}  // extern "C"
