// sampler_host.hpp -- what mass_adapt.hip, which sits above the sampler entry points, calls in mi_mcmc.hip, where these are defined: the common
// argument checks, the staging of a shard of chains, the fill of n_leapfrogs.
#pragma once

#include "host_common.hpp"

namespace mi {
namespace host {

int check_common(const mi_target* t, const mi_settings* s, const mi_chains* c, bool mass_allowed = false);
int fill_n_leap(uint64_t* dev_ptr, uint64_t n, uint64_t v, hipStream_t st);      // n_leapfrogs of a sampler whose kernel does not count; nullptr: nothing

// host <-> device staging of one mi_chains shard
struct StagedChains {
    DevBuf theta, draws, n_accept, step, n_leap, depth, mass, adapt, n_exec;
    mi_chains dev;   // device-pointer view
    bool exec_written = false;   // the kernel wrote n_leapfrogs_executed itself (nuts_memo.hpp); otherwise it is a copy of n_leapfrogs
};
int stage_in(const mi_chains* c, uint64_t d, uint64_t n_keep, StagedChains& sc, hipStream_t st, uint64_t n_total = 0);
int stage_out(const mi_chains* c, uint64_t d, uint64_t n_keep, StagedChains& sc, hipStream_t st, uint64_t n_total = 0);

}  // namespace host
}  // namespace mi
