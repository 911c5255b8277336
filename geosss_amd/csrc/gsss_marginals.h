// gsss_marginals.h -- per-target marginal histograms of a block of retained draws (gsss_target_marginals, include/gsss.h): the
// launcher that gsss_capi.hip calls after it has checked the arguments.  The kernels are in gsss_marginals.hip.
#pragma once
#include "gsss_device.h"

namespace gsss {

constexpr int kMarginalsMaxDirs = 32;        // directions per target
constexpr int kMarginalsMaxBins = 1024;      // bins of a series
constexpr int kMarginalsMaxCounters = 8192;  // series x bins per target: 32 KiB of 32-bit counters in LDS
constexpr int64_t kMarginalsMaxRows = (int64_t)1 << 23;  // rows of a block: 256 lanes x 2^23 rows < 2^32, a workgroup's LDS counter

// series per target: the directions and, with steps, the geodesic step
constexpr int64_t marginal_series(int n_dirs, bool steps) { return (int64_t)n_dirs + (steps ? 1 : 0); }

// ring: [ring_rows][d][n_chains]; the block is its rows first_row .. first_row + n_rows - 1, preceded (steps only) by n_hist <= 1
// rows of history at (first_row - 1) mod ring_rows.  dirs [n_chains / m][n_dirs][d]; count [n_chains / m][series][n_bins] is
// added to.  The current device is the buffers'.
int launch_target_marginals(const double *ring, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist,
                            int64_t n_chains, int d, int64_t m, const double *dirs, int n_dirs, int n_bins, bool steps,
                            int64_t *count, hipStream_t st);

}  // namespace gsss
