// Host build of geosss_amd/csrc/gsss_math.h for tests/test_acg_host.py: exp_fast and exp_fast_k side by side.
#include "../../geosss_amd/csrc/gsss_math.h"

extern "C" void t_exp_pair(const double *x, long n, double *plain, double *k)
{
    for (long i = 0; i < n; ++i) {
        plain[i] = gsss::fm::exp_fast(x[i]);
        k[i] = gsss::fm::exp_fast_k(x[i]);
    }
}
