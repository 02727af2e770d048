// Host scaffold shared by the solvers beside DORT (first_order.hip, second_order.hip, successive_order.hip,
// successive_order_active.hip, multifresnel.hip, nadir_lrm_altimetry.hip, nadir_sar_altimetry.hip): the error macro, the state base that owns a
// solver's device buffers and events, and the steps every entry point repeats -- pair list, upload of the smrt_batch
// arrays, sync, event times, table copies.  What differs between the solvers (kernels, chunk plans, launches, downloads)
// stays in their files; what they refuse is in solver_refusals.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <string>
#include <vector>

#include "dort_ctx.hpp"
#include "dort_host_common.hpp"

// For functions with a `smrt_dort_ctx* ctx` that return a negative value on error.
#define HIPCHK(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
            return -1;                                                                            \
        }                                                                                         \
    } while (0)

namespace solver_host {

// Base of a solver's state on the context.  A state names its device buffers as references into the pool
// (`DevBuf &stage = buf(), &out = buf();`), so that whatever a solver declares is freed with the state; the events are
// one pool for the fixed few of the two-kernel solvers and for the per-chunk ones of the successive-order solvers.
struct SolverState {
    std::deque<DevBuf> bufs;
    std::vector<hipEvent_t> ev;   // created on first use, recorded in order from 0 after rewind()
    size_t ev_used = 0;
    DevBuf& buf() { return bufs.emplace_back(); }
    void rewind() { ev_used = 0; }
    SolverState() = default;
    SolverState(const SolverState&) = delete;
    ~SolverState() {
        for (DevBuf& b : bufs) b.release();
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

// ... with the smrt_batch arrays every solver but the second-order one (which hands them to first order) uploads itself
struct InputState : SolverState {
    DevBuf &nl = buf(), &thick = buf(), &fv = buf(), &temp = buf(), &p1 = buf(), &p2 = buf(), &freq = buf(), &lw = buf(),
           &kind = buf(), &sub1 = buf(), &sub2 = buf(), &pairmap = buf();
};

// the body of smrt_launch::*_release: frees the state a context holds, if any
template <class State>
void release(State*& st) {
    delete st;
    st = nullptr;
}

// records the next event of the pool on the context's stream
inline int record(smrt_dort_ctx* ctx, SolverState* st) {
    if (st->ev_used == st->ev.size()) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        st->ev.push_back(e);
    }
    HIPCHK(hipEventRecord(st->ev[st->ev_used++], ctx->stream));
    return 0;
}

// waits for the event recorded last (what *_kernel_ms does before it reads the times)
inline int wait_recorded(smrt_dort_ctx* ctx, const SolverState* st) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(st->ev[st->ev_used - 1]));
    return 0;
}

// adds the milliseconds between the events i and j to *ms
inline int add_elapsed(smrt_dort_ctx* ctx, const SolverState* st, size_t i, size_t j, double* ms) {
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, st->ev[i], st->ev[j]));
    *ms += f;
    return 0;
}

inline int upload(smrt_dort_ctx* ctx, DevBuf& buf, const void* src, size_t bytes) {
    HIPCHK(buf.reserve(bytes));
    HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

// ... and sets the device pointer that reads it
template <class T>
int upload(smrt_dort_ctx* ctx, DevBuf& buf, const void* src, size_t bytes, T*& field) {
    if (upload(ctx, buf, src, bytes)) return -1;
    field = (T*)buf.p;
    return 0;
}

// room for `count` elements of a work or output buffer, and the device pointer that writes them
template <class T>
int reserve(smrt_dort_ctx* ctx, DevBuf& buf, size_t count, T*& field) {
    HIPCHK(buf.reserve(count * sizeof(T)));
    field = (T*)buf.p;
    return 0;
}

// the pair list of an *_upload_pairs call (smrt_host::refuse_pairs: null means all pairs, *n_pairs is set)
inline int check_pairs(smrt_dort_ctx* ctx, const int64_t* pairs, int64_t* n_pairs, int64_t all) {
    const char* why = smrt_host::refuse_pairs(pairs, n_pairs, all);
    if (why) ctx->err = why;
    return why ? -1 : 0;
}

// The arrays of a (validated) smrt_batch that the solvers read alike, into the state's buffers and the device batch `d`
// (FoBatch, SoBatch and MfBatch name these fields alike).  The substrate arrays go with d.sub_kind, which the caller has
// set; its temperature, the angles and everything else a solver reads on its own are the caller's to upload.
template <class Batch>
int upload_batch(smrt_dort_ctx* ctx, InputState* st, const smrt_batch* b, const int64_t* pairs, Batch& d) {
    const size_t S = b->n_snowpacks, L = b->n_layers_max, F = b->n_frequencies, SL = S * L * sizeof(double);
    if (upload(ctx, st->nl, b->n_layers, S * sizeof(int32_t), d.n_layers) || upload(ctx, st->thick, b->thickness, SL, d.thickness) ||
        upload(ctx, st->fv, b->frac_volume, SL, d.frac_volume) || upload(ctx, st->temp, b->temperature, SL, d.temperature) ||
        upload(ctx, st->p1, b->micro_p1, SL, d.p1) || upload(ctx, st->freq, b->frequency, F * sizeof(double), d.frequency))
        return -1;
    if (b->micro_p2 && upload(ctx, st->p2, b->micro_p2, SL, d.p2)) return -1;
    if (b->liquid_water && upload(ctx, st->lw, b->liquid_water, SL, d.liquid_water)) return -1;
    if (b->layer_kind && upload(ctx, st->kind, b->layer_kind, S * L * sizeof(int32_t), d.layer_kind)) return -1;
    // (the rough soils: their [S][2] parameters follow the [F][S] permittivities in both arrays, smrt_dort.h)
    const size_t sub_bytes = (F * S + (smrt_host::is_soil_substrate(d.sub_kind) ? 2 * S : 0)) * sizeof(double);
    if (d.sub_kind != SMRT_SUBSTRATE_NONE && (upload(ctx, st->sub1, b->substrate_p1, sub_bytes, d.sub_p1) ||
                                              upload(ctx, st->sub2, b->substrate_p2, sub_bytes, d.sub_p2)))
        return -1;
    if (pairs && upload(ctx, st->pairmap, pairs, (size_t)d.n_pairs * sizeof(int64_t), d.pair_map)) return -1;
    return 0;
}

// After the last upload of an *_upload_pairs call.  The copies read the caller's (pageable) arrays and the call's own
// vectors: wait for them, the arrays may go away or change after the call.
inline int uploads_done(smrt_dort_ctx* ctx) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// the *_sync exports
inline int32_t sync(smrt_dort_ctx* ctx) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The *_abi offset tables and the *_launch_info values: as many entries as fit `capacity` (none when out is null);
// returns the table's length.
template <class T, size_t N>
int32_t copy_table(const T (&table)[N], T* out, int32_t capacity) {
    for (int32_t i = 0; out && i < (int32_t)N && i < capacity; ++i) out[i] = table[i];
    return (int32_t)N;
}

}  // namespace solver_host
