// The smrt_batch arrays every solver beside DORT reads alike, bound to a described batch struct of the CPU drivers: the mirror
// of solver_host::upload_batch (smrt_amd/csrc/solver_host.hpp), templated the same way.  The substrate arrays go with
// d.sub_kind, as on the device; the pair map is copied (int64_t to the kernels' long long) and lives as long as this object.
// Angles, substrate temperature and everything else a solver reads on its own are the driver's to bind.
#pragma once
#include <cstdint>
#include <vector>

#include "../../smrt_amd/csrc/solver_describe.hpp"

namespace host_batch {

// the layer scalars a caller evaluated (smrt_batch.host_layer, host_iba_coeff): the batches of the first-order layer kernel
inline void bind_host_layers(const smrt_batch* b, smrt::FoBatch& d) { d.host_layer = b->host_layer; d.host_coeff = b->host_iba_coeff; }
template <class Batch> void bind_host_layers(const smrt_batch*, Batch&) {}

struct Inputs {
    std::vector<long long> pair_map;

    template <class Batch>
    void bind(const smrt_batch* b, const int64_t* pairs, Batch& d) {
        const solver_describe::InputExtents n = solver_describe::inputs(d, pairs != nullptr);
        d.n_layers = b->n_layers; d.layer_kind = b->layer_kind;
        d.thickness = b->thickness; d.frac_volume = b->frac_volume; d.temperature = b->temperature;
        d.p1 = b->micro_p1; d.p2 = b->micro_p2; d.frequency = b->frequency; d.liquid_water = b->liquid_water;
        if (n.substrate) { d.sub_p1 = b->substrate_p1; d.sub_p2 = b->substrate_p2; }
        if (pairs) { pair_map.assign(pairs, pairs + n.pair_map); d.pair_map = pair_map.data(); }
        bind_host_layers(b, d);
    }
};

}  // namespace host_batch
