// TEST INFRASTRUCTURE ONLY: the item lists of the launches per size class of rows (smrt_amd/csrc/dort_class_lists.hpp) under
// the fiber emulator, built the way smrt_dort_upload builds them -- count in the cost kernel's body, offsets on the host, fill
// per dispatch position -- and walked the way the kernels of k_prep_layer.hip walk them (class_item_of_block), next to what the
// full-grid launches visit (jacobi_item_of_block) and keep (prep_item_rows, from the rows the setup stage records).  Passive
// batches of the built-in emmodels, N <= 64.  Never loaded by smrt_amd.
#include "emu_lib.cpp"
#include "../../smrt_amd/csrc/dort_prep_layer.hpp"

// pair_map: null, or the pair_count listed pairs.  dispatch: null, or per chunk a permutation of the chunk-local pair slots.
// Out: rows_setup [pair_count][Lmax] stg.n as the setup kernel of every chunk left it (0: nothing staged); seg_offset / seg_count
// [chunks][3]; listed [pair_count * Lmax] the items the launches of (chunk, class) take through the lists, chunk-local, at
// seg_offset; full_count [chunks][3] and full [chunks][3][chunk_pairs * Lmax] the items the full-grid launch of (chunk, class)
// keeps, in its block order.  Returns the total length of the lists, -1 on a bad batch.
extern "C" long long smrt_emu_class_lists(const smrt_batch* b, const long long* pair_map, long long pair_count, long long chunk_pairs,
                                          const int* dispatch, int order, int* rows_setup, long long* seg_offset, long long* seg_count,
                                          int* listed, long long* full_count, int* full, long long* misses) {
    if (smrt_host::validate(b) || b->mode != SMRT_MODE_PASSIVE || b->n_max_stream > 32 || b->host_layer || b->substrate_kind) return -1;
    std::vector<double> gl(b->n_max_stream);
    smrt_host::gauss_legendre_positive(b->n_max_stream, gl.data(), nullptr);
    const int ostride = smrt_host::out_stride(b);
    std::vector<double> out((size_t)pair_count * ostride, 0.0), cost((size_t)pair_count, 0.0);
    std::vector<int32_t> status((size_t)pair_count, -9);
    unsigned long long miss = 0;
    DevBatch d{};
    d.S = b->n_snowpacks; d.Lmax = b->n_layers_max; d.F = b->n_frequencies; d.n_theta = b->n_theta;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.mode = b->mode; d.n_max_stream = b->n_max_stream;
    d.m_max = b->m_max; d.normalization = b->phase_normalization; d.rayleigh_jeans = b->rayleigh_jeans;
    d.pair_begin = 0; d.pair_count = pair_count; d.pair_map = pair_map;
    d.n_layers = b->n_layers; d.thickness = b->thickness; d.frac_volume = b->frac_volume;
    d.temperature = b->temperature; d.p1 = b->micro_p1; d.p2 = b->micro_p2 ? b->micro_p2 : b->micro_p1;
    d.frequency = b->frequency; d.theta = b->theta; d.gl_mu = gl.data(); d.phi = b->phi;
    d.layer_kind = b->layer_kind; d.liquid_water = b->liquid_water;
    d.host_modes = 1; d.host_ne = b->n_max_stream * 2;
    d.coherent = b->process_coherent_layers ? 1 : 0;
    d.layer_lo = 0; d.layer_hi = b->n_layers_max;
    d.out = out.data(); d.status = status.data(); d.class_miss = &miss;
    const long long Lmax = d.Lmax;
    // count: the body of dort_cost_kernel per pair slot of the upload
    std::vector<int> rows((size_t)(pair_count * Lmax), -7), counts((size_t)pair_count * kRowClasses, -7);
    {
        std::vector<double> lds((size_t)make_plan(d.n_max_stream, 2, d.Lmax, d.n_theta, 1, 0, 0, 1).total, NAN);
        for (long long p = 0; p < pair_count; ++p)
            emu::run_block(64, order, [&]() { dort_cost_pair<64>(d, p, lds.data(), cost.data(), rows.data(), counts.data()); });
    }
    // offsets, then fill per dispatch position
    d.dispatch = dispatch;
    const ClassListPlan plan = make_class_list_plan(counts.data(), dispatch, pair_count, chunk_pairs);
    std::vector<int> list((size_t)(pair_count * Lmax), -1);
    for (long long w = 0; w < pair_count; ++w) class_fill_pair(d.Lmax, chunk_pairs, dispatch, rows.data(), plan.pair_offset.data(), w, list.data());
    for (size_t i = 0; i < plan.seg_offset.size(); ++i) { seg_offset[i] = plan.seg_offset[i]; seg_count[i] = plan.seg_count[i]; }
    // every chunk: the setup kernel on the chunk's staging area, then its launches per class both ways
    const int recd = prep_record_doubles(d.n_max_stream);
    std::vector<double> rec((size_t)(chunk_pairs * Lmax) * recd, NAN), lds((size_t)make_plan(d.n_max_stream, 2, d.Lmax, d.n_theta, 9, 1, 0, 5).total, NAN);
    std::vector<int> stn((size_t)(chunk_pairs * Lmax));
    for (long long c = 0; c < plan.chunks; ++c) {
        const long long c0 = c * chunk_pairs, cn = std::min(chunk_pairs, pair_count - c0);
        DevBatch cb = d;   // like chunk_of (dort_hip.hip)
        cb.pair_begin = c0; cb.pair_count = cn; cb.out = d.out + c0 * ostride; cb.status = d.status + c0;
        if (dispatch) cb.dispatch = dispatch + c0;
        DevStage st{};
        st.n = stn.data(); st.rec = rec.data(); st.rec_stride = recd; st.vec_stride = 2 * d.n_max_stream;
        for (auto& x : stn) x = 0;
        for (long long w = 0; w < cn; ++w)
            emu::run_block(64, order, [&]() { dort_prep_setup_pair<64>(cb, dispatched_pair(cb, w), lds.data(), st); });
        for (long long i = 0; i < cn * Lmax; ++i) rows_setup[c0 * Lmax + i] = stn[(size_t)i];
        for (int k = 0; k < kRowClasses; ++k) {
            const int lo = k == 0 ? 0 : k == 1 ? 32 : 48, hi = k == 0 ? 32 : k == 1 ? 48 : 64;
            // through the list, like dort_prep_layer_kernel<.., LO, HI, ..>: lookup, then the kernel's own filter
            DevBatch cl = cb;
            cl.class_list = list.data() + plan.seg_offset[(size_t)c * kRowClasses + k];
            for (long long blk = 0; blk < plan.seg_count[(size_t)c * kRowClasses + k]; ++blk) {
                const long long item = class_item_of_block(cl, blk);
                listed[plan.seg_offset[(size_t)c * kRowClasses + k] + blk] = (int)item;
                const int r = prep_item_rows(cl, st, item);
                if (r <= lo || r > hi) emu::run_block(64, order, [&]() { class_list_left(cl, r); });
            }
            // the full grid
            long long n = 0;
            int* dst = full + ((size_t)c * kRowClasses + k) * (size_t)(chunk_pairs * Lmax);
            for (long long blk = 0; blk < cn * Lmax; ++blk) {
                const long long item = class_item_of_block(cb, blk);
                const int r = prep_item_rows(cb, st, item);
                if (r > lo && r <= hi) dst[n++] = (int)item;
            }
            full_count[(size_t)c * kRowClasses + k] = n;
        }
    }
    *misses = (long long)miss;
    return plan.total;
}
