// Compact item lists for the launches that take one size class of rows each (the per-layer prep of k_prep_layer.hip and the
// gram / tridiag / vectors kernels of k_eig.hip; passive mode, N <= 64): instead of a grid over every (pair, layer) item of a
// pipeline pass, whose workgroups look up their item's rows and mostly leave, a launch is as long as the list of its class.
//
// The class of an item is a function of the uploaded inputs -- the stream count pair_setup gives the layer -- so the lists are
// built once per upload, next to the pair costs and the dispatch order, and hold for every launch of that upload:
//   count   (device, the cost kernel: class_count_pair)  rows of every item as the setup stage will record them, and per pair
//           the number of its items in each class; the counts come back with the costs
//   offsets (host, with the dispatch order it has just sorted: make_class_list_plan)  where the items of every workgroup's
//           pair start in the list of each class; the lists of a pipeline chunk are contiguous: ordered by (chunk, class,
//           dispatch position of the pair, layer) -- within a class the order jacobi_item_of_block visits the items in
//   fill    (device: class_fill_pair)  every pair writes its items behind its own offsets: no atomics, the same list each time
// A list only decides which workgroups are dispatched; what a workgroup computes, and whether (status, pair_done, layers beyond
// the snowpack, rows in class), stays with the filters of the kernels.  Plain C++ apart from SMRT_DEV: the CPU build of the
// device code (tests/hostemu) builds and walks the same lists.
// Part of the DORT device code (see dort_device.hpp for the overview and the reference map).
#pragma once
#include <vector>

#include "dort_layout.hpp"

namespace smrt {

// Size classes by row count, those of k_prep_layer.hip and k_eig.hip: (0, 32], (32, 48], (48, 64]
constexpr int kRowClasses = 3;
SMRT_HD int row_class(int rows) { return rows <= 0 ? -1 : rows <= 32 ? 0 : rows <= 48 ? 1 : rows <= 64 ? 2 : -1; }
// launches <LO, HI> -> index of the class
template <int LO, int HI>
constexpr int row_class_index() {
    static_assert((LO == 0 && HI == 32) || (LO == 32 && HI == 48) || (LO == 48 && HI == 64), "not a size class of rows");
    return LO == 0 ? 0 : LO == 32 ? 1 : 2;
}

// rows the setup stage of the prep records for layer l of a pair (stg.n[item]), from the tables pair_setup left in LDS
SMRT_DEV int setup_item_rows(const Lds& s, int l) { return 2 * (int)s.nl[l]; }

// count: after pair_setup of pair slot p returned st (one thread).  rows [pair_count][Lmax] (0: no item -- beyond the
// snowpack's layers, or a pair the setup rejects), counts [pair_count][kRowClasses]
SMRT_DEV void class_count_pair(const DevBatch& b, const Lds& s, int st, long long p, int* rows, int* counts) {
    const int L = (st == ST_OK) ? s.ints[6] : 0;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int l = 0; l < b.Lmax; ++l) {
        const int r = (l < L) ? setup_item_rows(s, l) : 0;
        rows[p * b.Lmax + l] = r;
        const int k = row_class(r);
        c0 += (k == 0); c1 += (k == 1); c2 += (k == 2);
    }
    counts[p * kRowClasses] = c0; counts[p * kRowClasses + 1] = c1; counts[p * kRowClasses + 2] = c2;
}

// offsets.  pair_offset [pair_count][kRowClasses], by DISPATCH POSITION w of the whole upload (chunk * chunk_pairs + position
// in the chunk): index in `list` of the first item of class k of the pair that workgroup takes.  seg_offset / seg_count
// [chunks][kRowClasses]: the contiguous segment of a chunk's items of a class.
struct ClassListPlan {
    long long pair_count = 0, chunk_pairs = 0, chunks = 0, total = 0;
    std::vector<long long> pair_offset, seg_offset, seg_count;
    bool empty() const { return chunks == 0; }
    void clear() { *this = ClassListPlan(); }
};
// counts: by pair slot of the upload; dispatch: [pair_count] chunk-local pair slot of every dispatch position, or null
inline ClassListPlan make_class_list_plan(const int* counts, const int* dispatch, long long pair_count, long long chunk_pairs) {
    ClassListPlan plan;
    plan.pair_count = pair_count; plan.chunk_pairs = chunk_pairs;
    plan.chunks = (pair_count + chunk_pairs - 1) / chunk_pairs;
    plan.pair_offset.assign((size_t)pair_count * kRowClasses, 0);
    plan.seg_offset.assign((size_t)plan.chunks * kRowClasses, 0);
    plan.seg_count.assign((size_t)plan.chunks * kRowClasses, 0);
    long long at = 0;
    for (long long c = 0; c < plan.chunks; ++c) {
        const long long c0 = c * chunk_pairs, cn = (chunk_pairs < pair_count - c0) ? chunk_pairs : pair_count - c0;
        for (int k = 0; k < kRowClasses; ++k) {
            plan.seg_offset[(size_t)c * kRowClasses + k] = at;
            for (long long i = 0; i < cn; ++i) {
                const long long slot = c0 + (dispatch ? (long long)dispatch[c0 + i] : i);
                plan.pair_offset[(size_t)(c0 + i) * kRowClasses + k] = at;
                at += counts[slot * kRowClasses + k];
            }
            plan.seg_count[(size_t)c * kRowClasses + k] = at - plan.seg_offset[(size_t)c * kRowClasses + k];
        }
    }
    plan.total = at;
    return plan;
}

// fill: dispatch position w of the upload writes the items of its pair, layers ascending, as indices local to its chunk
// (item = pair slot in the chunk * Lmax + layer: what the kernels of the chunk index the staging area with)
SMRT_DEV void class_fill_pair(int Lmax, long long chunk_pairs, const int* dispatch, const int* rows, const long long* pair_offset, long long w, int* list) {
    const long long c0 = (w / chunk_pairs) * chunk_pairs;
    const long long slot = dispatch ? (long long)dispatch[w] : w - c0;
    long long at[kRowClasses];
    for (int k = 0; k < kRowClasses; ++k) at[k] = pair_offset[w * kRowClasses + k];
    for (int l = 0; l < Lmax; ++l) {
        const int k = row_class(rows[(c0 + slot) * Lmax + l]);
        if (k >= 0) list[at[k]++] = (int)(slot * Lmax + l);
    }
}

}  // namespace smrt
