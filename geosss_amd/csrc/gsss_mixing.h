// gsss_mixing.h -- per-target step length, hopping and mode occupancy of a block of retained draws (gsss_target_mixing,
// include/gsss.h): the launcher that gsss_capi.hip calls after it has checked the arguments.  The kernels are in gsss_mixing.hip.
#pragma once
#include "gsss_device.h"

namespace gsss {

constexpr int kMixingMaxModes = 16;  // the batch's own limit on mixture terms

// int64 counters per target: draws, pairs, hops, K mode counts and, with transitions, K x K pair counts [mode before][mode after]
constexpr int64_t mixing_counters(int n_modes, bool transitions)
{
    return 3 + (int64_t)n_modes + (transitions ? (int64_t)n_modes * n_modes : 0);
}

// ring: [ring_rows][d][n_chains]; the block is its rows first_row .. first_row + n_rows - 1, preceded by n_hist <= 1 rows of
// history at (first_row - 1) mod ring_rows.  dirs [n_chains / m][1 + n_modes][d]; step [n_chains / m][2] and count
// [n_chains / m][mixing_counters] are added to.  The current device is the buffers'.
int launch_target_mixing(const double *ring, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist, int64_t n_chains,
                         int d, int64_t m, const double *dirs, int n_modes, bool transitions, double *step, int64_t *count,
                         hipStream_t st);

}  // namespace gsss
