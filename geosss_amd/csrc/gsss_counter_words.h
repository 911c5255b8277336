// The Philox counter words of a launch that stays inside one block of 2^32 chain ids and one of 2^32 step ids (host code only, no
// HIP: tests/cpp/counter_words_host.cpp builds it with g++).
//
// A draw's counter is (block, step low, chain low, chain high 16 | step high 16 << 16) with chain = chain_offset + c for the
// launch's chain c in [0, n_chains) and step = step_offset + s for its step count s in [0, n_steps] (a chain that has made all its
// steps holds s = n_steps).  While neither sum carries out of its low word over those ranges, the high words are the offsets'
// own: word 3 is one constant for the launch, and words 1 and 2 are 32-bit sums of the offsets' low words and s / c.  The lane
// kernels (screened_kernel, fast_kernel) form their counters that way under RunBlock::ctr32; every other launch, and every
// other kernel, adds in 64 bits (PhiloxDraws::init / begin_step, gsss_device.h).
#pragma once
#include <stdint.h>

namespace gsss {

struct CounterWords {
    int32_t ok;         // the launch stays inside one block of either kind: the three words below hold
    uint32_t chain_lo;  // word 2 of chain c is chain_lo + c
    uint32_t step_lo;   // word 1 of step count s is step_lo + s
    uint32_t c3;        // word 3
};

// [offset, offset + span] lies inside one block of 2^32 ids (span >= 0; the sum does not wrap 64 bits: the launch is refused
// far below that, at 2^48)
inline bool one_block32(uint64_t offset, int64_t span)
{
    return span >= 0 && (uint64_t)span <= 0xFFFFFFFFull - (offset & 0xFFFFFFFFull);
}

inline CounterWords counter_words(uint64_t chain_offset, int64_t n_chains, uint64_t step_offset, int64_t n_steps)
{
    CounterWords w{};
    // chains chain_offset .. chain_offset + n_chains - 1 (an empty launch draws nothing), step ids step_offset .. step_offset + n_steps
    w.ok = (n_chains >= 1 && one_block32(chain_offset, n_chains - 1) && one_block32(step_offset, n_steps)) ? 1 : 0;
    w.chain_lo = (uint32_t)chain_offset;
    w.step_lo = (uint32_t)step_offset;
    w.c3 = (uint32_t)((chain_offset >> 32) & 0xFFFFu) | ((uint32_t)((step_offset >> 32) & 0xFFFFu) << 16);
    return w;
}

// a launch's kept rows are addressed in 32 x 32 -> 64 bit arithmetic by the lane kernels (kept_row, gsss_device.h): the row
// stride keep_rows d of the chain-major layout, and rows d of either layout, stay below 2^31
inline bool kept_rows_fit32(int64_t keep_rows, int64_t n_steps, int64_t thin, int32_t d)
{
    const int64_t rows = thin >= 1 ? n_steps / thin : 0;
    return keep_rows < (1ll << 31) && keep_rows * (int64_t)d < (1ll << 31) && rows * (int64_t)d < (1ll << 31);
}

}  // namespace gsss
