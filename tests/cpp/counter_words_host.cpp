// Host build of geosss_amd/csrc/gsss_counter_words.h for tests/test_counter_words.py: the rule by which a launch's Philox counter
// words are formed once (RunBlock::ctr32) and the bound on the kept rows of the lane kernels, no HIP anywhere.
#include "../../geosss_amd/csrc/gsss_counter_words.h"

extern "C" int t_counter_words(uint64_t chain_offset, int64_t n_chains, uint64_t step_offset, int64_t n_steps, uint32_t *words)
{
    const gsss::CounterWords w = gsss::counter_words(chain_offset, n_chains, step_offset, n_steps);
    words[0] = w.chain_lo;
    words[1] = w.step_lo;
    words[2] = w.c3;
    return w.ok;
}

extern "C" int t_kept_rows_fit32(int64_t keep_rows, int64_t n_steps, int64_t thin, int32_t d)
{
    return gsss::kept_rows_fit32(keep_rows, n_steps, thin, d) ? 1 : 0;
}
