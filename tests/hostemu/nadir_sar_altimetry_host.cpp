// The device arithmetic of the nadir SAR altimetry solver (smrt_amd/csrc/nadir_sar_altimetry_kernel.hpp) compiled for the CPU:
// a "workgroup" of one thread, scans as running sums.  Built by tests/host_build.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_sar_host.so nadir_sar_altimetry_host.cpp
#include <cstdint>
#include <vector>

#include "../../smrt_amd/csrc/solver_refusals.hpp"
#include "host_batch.hpp"

using namespace smrt;

// Same batch, parameters and outputs as smrt_sar_run_pairs over every pair, without a context.  Returns 0, or -1 (refused).
extern "C" __attribute__((visibility("default")))
int32_t smrt_sar_host_run(const smrt_batch* b, const smrt_sar_params* p, double* out, int32_t* status, double* z_gate,
                          double* layer_out, double* vertical, double* echo) {
    if (!out || !status || !z_gate || !layer_out || !vertical || !echo) return -1;
    if (solver_refusals::nadir_sar_altimetry(b, p)) return -1;
    const long long NP = b->n_snowpacks;
    host_batch::Inputs in;
    smrt_sar_params dinardo = *p;   // (this library runs the route of Dinardo18 whatever the parameters name)
    dinardo.delay_doppler_model = SMRT_SAR_DINARDO18;
    SarBatch d = solver_describe::nadir_sar_altimetry(b, &dinardo, NP);
    LrmBatch& lb = d.lrm;
    FoBatch& fo = lb.fo;
    in.bind(b, nullptr, fo);
    const solver_describe::SarExtents n = solver_describe::extents(d);
    lb.itf = p->boundary_values;
    d.tab_sigma = p->table_sigma; d.tab_index = p->table_index; d.row_map = p->row_map;
    std::vector<double> stage(n.lrm.stage, 0.0), bs(n.lrm.bs, 0.0), prefix(n.lrm.prefix, 0.0), tables(n.tables);
    std::vector<unsigned char> lds(n.lrm.lds_vertical + n.lds_combine);
    fo.stage = stage.data(); fo.layer_out = layer_out;
    lb.bs = bs.data(); lb.prefix = prefix.data(); lb.vsd = vertical; lb.z_gate = z_gate; lb.status = status;
    d.tables = tables.data(); d.echo = echo; d.out = out;
    LrmLane ln{0, 1, nullptr};
    for (long long i = 0; i < NP; ++i)
        for (int l = 0; l < fo.Lmax; ++l) lrm_layer_item(lb, i, l);
    for (long long i = 0; i < NP; ++i) { lrm_vertical_pair(lb, i, ln, lds.data()); sar_boundary_pair(d, i, 0, 1); }
    for (long long k = 0; k < (long long)d.n_tab * lb.N * d.ND; ++k) sar_table_item(d, k);
    for (long long i = 0; i < NP; ++i)
        for (int bin = 0; bin < d.ndoppler; ++bin) sar_combine_item(d, i, bin, 0, 1, lds.data());
    return 0;
}

// f0 and f1 of Dinardo et al. 2018 as the kernels compute them (held to scipy.special.ive by the tests)
extern "C" __attribute__((visibility("default"))) double smrt_sar_host_f0(double xi) { return sar_f0(xi); }
extern "C" __attribute__((visibility("default"))) double smrt_sar_host_f1(double xi) { return sar_f1(xi); }
// what the C ABI answers to a batch before any device work: the message, or null
extern "C" __attribute__((visibility("default"))) const char* smrt_sar_host_refusal(const smrt_batch* b, const smrt_sar_params* p) {
    return solver_refusals::nadir_sar_altimetry(b, p);
}
