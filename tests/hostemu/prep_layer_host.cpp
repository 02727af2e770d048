// TEST INFRASTRUCTURE ONLY: the two prep stages of the LDS-resident passive pipeline side by side under the fiber
// emulator -- one workgroup per pair (dort_pair_passive MODE 1) and the per-layer prep (dort_prep_layer.hpp: pair setup,
// then one workgroup per item and size class) -- with the staging area as each of them leaves it.  The rest of the
// pipeline (symmetric eigensolver, Rayleigh closed form, strip finish kernel on four wavefronts, prune rounds) is
// emu_lib.cpp's, included as it is.  Never loaded by smrt_amd.
#include "emu_lib.cpp"
#include "../../smrt_amd/csrc/dort_prep_layer.hpp"

// The per-layer prep of one pair as k_prep_layer.hip launches it: setup, then the pair's items through every size class
// (an item of another class leaves at once)
template <int LO, int HI>
static long run_layer_class(DevBatch& d, const DevStage& st, long long item, int order, std::vector<double>& lds) {
    const int rows = prep_item_rows(d, st, item);
    if (rows <= LO || rows > HI) return 0;
    lds.assign((size_t)make_plan(HI / 2, 2, 0, 0, 9, 1, 0, 4).total, NAN);
    return emu::run_block(256, order, [&]() { dort_prep_layer_item<256, HI>(d, st, item, lds.data()); });
}
static long run_prep_layers(DevBatch& d, const DevStage& st, long long p, int order) {
    std::vector<double> lds((size_t)make_plan(d.n_max_stream, 2, d.Lmax, d.n_theta, 9, 1, 0, 5).total, NAN);
    long nb = emu::run_block(64, order, [&]() { dort_prep_setup_pair<64>(d, p, lds.data(), st); });
    for (int l = d.layer_lo; l < d.layer_hi; ++l) {
        const long long item = p * d.Lmax + l;
        nb += run_layer_class<0, 32>(d, st, item, order, lds);
        nb += run_layer_class<32, 48>(d, st, item, order, lds);
        nb += run_layer_class<48, 64>(d, st, item, order, lds);
    }
    return nb;
}

// Passive batch of the built-in emmodels (no host arrays, no substrate, no atmosphere), N <= 64, through prep ->
// eigensolver -> strip finish kernel.  per_layer: which prep.  stage_*: the staging area as the prep of every round left it,
// [pair_count * Lmax] items of (NMAX * LD, NMAX * LD, NMAX, 1024) doubles and one int.
extern "C" int smrt_emu_prep_run(const smrt_batch* b, int per_layer, int order, double* out, int32_t* status,
                                 double* stage_L, double* stage_B, double* stage_d, double* stage_inv, int* stage_n) {
    if (smrt_host::validate(b) || b->mode != SMRT_MODE_PASSIVE || b->n_max_stream > 32 || b->host_layer || b->substrate_kind) return -1;
    const LdsPlan plan = make_plan(b->n_max_stream, 2, b->n_layers_max, b->n_theta, 9, 1, 0, 0, 0);
    std::vector<double> gl(b->n_max_stream);
    smrt_host::gauss_legendre_positive(b->n_max_stream, gl.data(), nullptr);
    DevBatch d{};
    d.S = b->n_snowpacks; d.Lmax = b->n_layers_max; d.F = b->n_frequencies; d.n_theta = b->n_theta;
    d.emmodel = b->emmodel; d.micro = b->microstructure; d.mode = b->mode; d.n_max_stream = b->n_max_stream;
    d.m_max = b->m_max; d.normalization = b->phase_normalization; d.rayleigh_jeans = b->rayleigh_jeans;
    d.pair_begin = 0; d.pair_count = (long long)b->n_snowpacks * b->n_frequencies;
    d.n_layers = b->n_layers; d.thickness = b->thickness; d.frac_volume = b->frac_volume;
    d.temperature = b->temperature; d.p1 = b->micro_p1; d.p2 = b->micro_p2 ? b->micro_p2 : b->micro_p1;
    d.frequency = b->frequency; d.theta = b->theta; d.gl_mu = gl.data(); d.phi = b->phi;
    d.layer_kind = b->layer_kind; d.liquid_water = b->liquid_water;
    d.host_modes = 1; d.host_ne = b->n_max_stream * 2;
    d.coherent = b->process_coherent_layers ? 1 : 0;
    d.prune_tau = (b->prune_optical_depth > 0.0) ? b->prune_optical_depth : 0.0;
    d.layer_lo = 0; d.layer_hi = b->n_layers_max;
    d.jacobi_skip2 = SMRT_JACOBI_REG_SKIP_COS2; d.jacobi_exit2 = SMRT_JACOBI_REG_EXIT_COS2;
    d.out = out; d.status = status;
    const bool strip = !d.coherent;   // where the library runs the strip finish kernel; else the two-slot one
    d.rayleigh_direct = (strip && (d.layer_kind != nullptr || em_has_rayleigh_phase(d.emmodel))) ? 1 : 0;
    const size_t items = (size_t)d.pair_count * d.Lmax;
    Staging sg(items, plan);
    std::vector<double> rec(items * (size_t)prep_record_doubles(d.n_max_stream), NAN);
    sg.st.rec = rec.data(); sg.st.rec_stride = prep_record_doubles(d.n_max_stream);
    std::vector<double> lds((size_t)plan.total + finish_strip_lds_doubles(d.n_max_stream, d.Lmax, 4)), jl;
    const size_t mat = (size_t)plan.NMAX * plan.LD;
    auto snapshot = [&](long long p) {   // this round's items of the pair, as the prep left them
        for (int l = d.layer_lo; l < d.layer_hi; ++l) {
            const size_t it = (size_t)p * d.Lmax + l;
            memcpy(stage_L + it * mat, sg.L.data() + it * mat, mat * sizeof(double));
            memcpy(stage_B + it * mat, sg.B.data() + it * mat, mat * sizeof(double));
            memcpy(stage_d + it * plan.NMAX, sg.d.data() + it * plan.NMAX, plan.NMAX * sizeof(double));
            memcpy(stage_inv + it * 1024, sg.inv.data() + it * 1024, 1024 * sizeof(double));
            stage_n[it] = sg.n[it];
        }
    };
    for (size_t it = 0; it < items; ++it) stage_n[it] = -1;
    run_rounds(d, order, 1, sg,
        [&](long long p) { long nb;
                           if (per_layer) nb = run_prep_layers(d, sg.st, p, order);
                           else { for (auto& x : lds) x = NAN; nb = emu::run_block(256, order, [&]() { dort_pair_passive<256, 1, 1>(d, p, lds.data(), nullptr, &sg.st); }); }
                           snapshot(p);
                           return nb; },
        [&](long long it) { return run_jacobi_classes(d, sg.st, it, 2, order, jl); },
        [&](long long p) { for (auto& x : lds) x = NAN;
                           if (!strip) return emu::run_block(256, order, [&]() { dort_pair_passive<256, 1, 3>(d, p, lds.data(), nullptr, &sg.st); });
                           return d.rayleigh_direct ? emu::run_block(256, order, [&]() { dort_pair_passive_strip4<true>(d, p, lds.data(), sg.st); })
                                                   : emu::run_block(256, order, [&]() { dort_pair_passive_strip4<false>(d, p, lds.data(), sg.st); }); });
    return 0;
}
