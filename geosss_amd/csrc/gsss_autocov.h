// gsss_autocov.h -- per-target lagged products of a block of retained draws (gsss_target_autocov, include/gsss.h): the launcher
// that gsss_capi.hip calls after it has checked the arguments.  The kernels are in gsss_autocov.hip.
#pragma once
#include "gsss_device.h"

namespace gsss {

constexpr int kAutocovMaxLags = 64;

// accumulated doubles per (target, series): (C, P, Q) for the lags 0 .. n_lags
constexpr int64_t autocov_sums(int n_lags) { return 3 * ((int64_t)n_lags + 1); }

// ring: [ring_rows][d][n_chains]; the block is its rows first_row .. first_row + n_rows - 1, preceded by n_hist <= n_lags rows of
// history at (first_row - 1 - i) mod ring_rows.  acc [n_chains / m][d][n_lags + 1][3] is added to.  The current device is the
// buffers'.
int launch_target_autocov(const double *ring, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist, int64_t n_chains,
                          int d, int64_t m, int n_lags, double *acc, hipStream_t st);

}  // namespace gsss
