// Host build of geosss_amd/csrc/gsss_fast_select.h for tests/test_acg_host.py: the pick of an angular central Gaussian launch
// (or of any other kind, for comparison) and its name, no HIP anywhere.
#include "../../geosss_amd/csrc/gsss_fast_select.h"

// GSSS_OK / GSSS_E_UNSUPPORTED; name (empty when unsupported), lane and the pick's family
extern "C" int t_acg_select(int kind, int d, int k, int screen, int spread, int numpy, int replay, int stats, int batch, char *name, int n,
                            int *lane, int *family)
{
    gsss::FastAsk a{};
    a.kind = kind;
    a.d = d;
    a.k = k;
    a.screen = screen;
    a.spread = spread != 0;
    a.numpy = numpy != 0;
    a.replay = replay != 0;
    a.stats = stats != 0;
    a.batch = batch != 0;
    a.curve_tail = 1;
    gsss::FastPick p;
    const int rc = gsss::fast_select(a, p);
    name[0] = 0;
    *lane = 0;
    *family = -1;
    if (rc == GSSS_OK) {
        gsss::fast_name(p, name, (size_t)n);
        *lane = p.lane ? 1 : 0;
        *family = p.family;
    }
    return rc;
}
