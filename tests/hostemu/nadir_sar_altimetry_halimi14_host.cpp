// The device arithmetic of the nadir SAR altimetry solver (smrt_amd/csrc/nadir_sar_altimetry_kernel.hpp) compiled for the CPU with
// BOTH delay-Doppler models: what nadir_sar_altimetry_host.cpp does for Dinardo18, and the table stage and the map of Halimi et
// al. 2014 as smrt_sar_launch runs them.  A "workgroup" is one thread.  Built by tests/host_build.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_sar_halimi14_host.so nadir_sar_altimetry_halimi14_host.cpp
#include <cstdint>
#include <vector>

#include "../../smrt_amd/csrc/solver_refusals.hpp"
#include "host_batch.hpp"

using namespace smrt;

// Same batch, parameters and outputs as smrt_sar_run_pairs over every pair, without a context.  `table` (may be null) receives the
// first table of Halimi14 as the reference lays it out, [ngate x oversampling_time][ndoppler x oversampling_doppler].
// Returns 0, or -1 (refused).
extern "C" __attribute__((visibility("default")))
int32_t smrt_sar_host_run_table(const smrt_batch* b, const smrt_sar_params* p, double* out, int32_t* status, double* z_gate,
                                double* layer_out, double* vertical, double* echo, double* table) {
    if (!out || !status || !z_gate || !layer_out || !vertical || !echo) return -1;
    if (solver_refusals::nadir_sar_altimetry(b, p)) return -1;
    const long long NP = b->n_snowpacks;
    host_batch::Inputs in;
    SarBatch d = solver_describe::nadir_sar_altimetry(b, p, NP);
    LrmBatch& lb = d.lrm;
    FoBatch& fo = lb.fo;
    in.bind(b, nullptr, fo);
    const solver_describe::SarExtents n = solver_describe::extents(d);
    const bool h14 = d.model == kSarHalimi14;
    lb.itf = p->boundary_values;
    d.tab_sigma = p->table_sigma; d.tab_index = p->table_index; d.row_map = p->row_map;
    std::vector<double> stage(n.lrm.stage, 0.0), bs(n.lrm.bs, 0.0), prefix(n.lrm.prefix, 0.0), tables(n.tables);
    std::vector<double> doppler(n.h14_doppler), kernel(n.h14_kernel);
    // (each stage has exactly the LDS the launch gives it: a read past it is a read past the vector)
    std::vector<unsigned char> lds_vertical(n.lrm.lds_vertical), lds_combine(n.lds_combine);
    fo.stage = stage.data(); fo.layer_out = layer_out;
    lb.bs = bs.data(); lb.prefix = prefix.data(); lb.vsd = vertical; lb.z_gate = z_gate; lb.status = status;
    d.tables = tables.data(); d.echo = echo; d.out = out;
    d.h14_doppler = doppler.data(); d.h14_kernel = kernel.data();
    LrmLane ln{0, 1, nullptr};
    for (long long i = 0; i < NP; ++i)
        for (int l = 0; l < fo.Lmax; ++l) lrm_layer_item(lb, i, l);
    for (long long i = 0; i < NP; ++i) { lrm_vertical_pair(lb, i, ln, lds_vertical.data()); sar_boundary_pair(d, i, 0, 1); }
    if (h14) {
        std::vector<unsigned char> l1(n.lds_h14_doppler), l2(n.lds_h14_kernel), l3(n.lds_h14_delay);
        for (int k = 0; k < d.N_wide; ++k) sar_h14_doppler_row(d, k, 0, 1, l1.data());
        for (int t = 0; t < d.n_tab; ++t) sar_h14_kernel_table(d, t, 0, 1, l2.data());
        for (int t = 0; t < d.n_tab; ++t)
            for (int c = 0; c < d.ND; ++c) sar_h14_delay_column(d, t, c, 0, 1, l3.data());
        for (int k = 0; table && k < lb.N; ++k)
            for (int c = 0; c < d.ND; ++c) table[(size_t)k * d.ND + c] = tables[(size_t)c * lb.N + k];
    } else {
        for (long long k = 0; k < (long long)d.n_tab * lb.N * d.ND; ++k) sar_table_item(d, k);
    }
    for (long long i = 0; i < NP; ++i)
        for (int bin = 0; bin < d.ndoppler; ++bin) {
            if (h14) sar_combine_model<kSarHalimi14>(d, i, bin, 0, 1, lds_combine.data());
            else sar_combine_model<kSarDinardo18>(d, i, bin, 0, 1, lds_combine.data());
        }
    return 0;
}

extern "C" __attribute__((visibility("default")))
int32_t smrt_sar_host_run(const smrt_batch* b, const smrt_sar_params* p, double* out, int32_t* status, double* z_gate,
                          double* layer_out, double* vertical, double* echo) {
    return smrt_sar_host_run_table(b, p, out, status, z_gate, layer_out, vertical, echo, nullptr);
}

// what the C ABI answers to a batch before any device work: the message, or null
extern "C" __attribute__((visibility("default"))) const char* smrt_sar_host_refusal(const smrt_batch* b, const smrt_sar_params* p) {
    return solver_refusals::nadir_sar_altimetry(b, p);
}
