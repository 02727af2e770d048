// What the solvers beside DORT refuse (smrt_amd/csrc/solver_refusals.hpp and the checks they share in dort_host_common.hpp),
// behind one C entry point for the CPU tests.  Built by tests/test_solver_refusals_cpu.py:
//   g++ -O2 -std=c++17 -shared -fPIC -DSMRT_HOST_EMU -I tests/hostemu -o libsmrt_solver_refusals_host.so solver_refusals_host.cpp
#include <cstdint>

#include "../../smrt_amd/csrc/solver_refusals.hpp"
#include "../../include/smrt_dort.h"

// What a solver answers to a batch it refuses, as its *_upload_pairs would before any device work: the solver's own
// refusals, then the pair list (null: every pair); null when it takes both.  solver: 0 first_order, 1 second_order,
// 2 successive_order, 3 successive_order_active, 4 multifresnel, 5 nadir_lrm_altimetry.  The batch's theta stands for the
// incidence angles (3) and the sensor cosines (4), which are only looked at for being there; altimetry gets a valid sensor
// around ngate and oversampling.
extern "C" __attribute__((visibility("default")))
const char* smrt_emu_solver_refusal(int solver, const smrt_batch* b, int n_iteration_max, double relative_tolerance, int n_theta_inc,
                                    int incident_npol, int m_max, int ngate, int oversampling, const int64_t* pairs, int64_t n_pairs) {
    const double* angles = b ? b->theta : nullptr;
    smrt_lrm_params p{};
    p.altitude = 800e3; p.pulse_bandwidth = 320e6; p.antenna_gain = 1.0; p.gamma = 1e-4; p.pulse_sigma = 1.0;
    p.ngate = ngate; p.oversampling = oversampling; p.n_mu = 1; p.shift = 1;
    const char* why = nullptr;
    switch (solver) {
        case 0: why = solver_refusals::first_order(b, nullptr); break;
        case 1: why = solver_refusals::second_order(b); if (!why) why = solver_refusals::first_order(b, nullptr); break;
        case 2: why = solver_refusals::successive_order(b, n_iteration_max, relative_tolerance); break;
        case 3: why = solver_refusals::successive_order_active(b, n_iteration_max, relative_tolerance, n_theta_inc, angles, incident_npol, m_max); break;
        case 4: why = solver_refusals::multifresnel(b, angles, 10.0, 0); break;
        case 5: why = solver_refusals::nadir_lrm_altimetry(b, &p); break;
        default: return "unknown solver";
    }
    return why ? why : smrt_host::refuse_pairs(pairs, &n_pairs, (int64_t)b->n_snowpacks * b->n_frequencies);
}
