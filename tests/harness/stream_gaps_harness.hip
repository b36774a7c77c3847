// TEST INFRASTRUCTURE ONLY -- not part of the product, never loaded by seqikpy_amd.
//
// Runs the two rules skip mode adds for streams (csrc/seqik_gaps.hpp) on the HOST: which compact slot of a solved slab
// becomes a chain's carried state (the rule the carry kernel of csrc/seqik_stream.hip applies per lane), and the seed
// state.  With tests/harness/gaps_harness.hip and tests/harness/host_harness.hip the CPU-only tier walks a carried skip
// stream slab by slab.  Built by tests/stream_gaps_model.py with `hipcc --offload-host-only`.
#include "../../sequential-inverse-kinematics_amd/csrc/seqik_gaps.hpp"

extern "C" int64_t harness_carry_slot(int64_t n_valid) { return seqik::gaps_carry_slot(n_valid); }

// cangles [n][7] of one chain's solved compact slab; state [7] is updated in place
extern "C" void harness_carry_chain(const double *cangles, int64_t n_valid, double *state)
{
    seqik::gaps_carry_chain(cangles, n_valid, state);
}

extern "C" void harness_seed_state(const SeqikLegParams *leg, int32_t generic, double *state)
{
    seqik::stream_seed_state(*leg, generic != 0, state);
}
