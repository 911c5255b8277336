// gsss_moments.h -- per-target moments of a block of retained draws (gsss_target_moments, include/gsss.h): the launcher that
// gsss_capi.hip calls after it has checked the arguments.  The kernels are in gsss_moments.hip.
#pragma once
#include "gsss_device.h"

namespace gsss {

constexpr int kMomentsMaxFullDim = 16;  // the full triangle is kept in registers up to here (the batch fast kernels' limit)

// accumulated rows per target behind the count row: d sums, then the triangle or the diagonal
constexpr int64_t moments_sums(int d, bool diag) { return (int64_t)d + (diag ? (int64_t)d : (int64_t)d * (d + 1) / 2); }

// x: [n_rows][d][n_chains] (chain_rows == 0) or rows 0 .. n_rows - 1 of every chain's run of chain_rows rows in a
// [n_chains][chain_rows][d] array.  acc [n_chains / m][1 + moments_sums] and chain_sum (NULL or [d][n_chains]) are added to.
// The current device is the buffers'.
int launch_target_moments(const double *x, int64_t n_rows, int64_t n_chains, int d, int64_t chain_rows, int64_t m, bool diag,
                          double *acc, double *chain_sum, hipStream_t st);

}  // namespace gsss
