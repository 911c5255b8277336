// Host build of geosss_amd/csrc/gsss_fast_select.h for tests/test_fast_select.py: the selection and its name, no HIP anywhere.
#include "../../geosss_amd/csrc/gsss_fast_select.h"

// GSSS_OK / GSSS_E_UNSUPPORTED; name (empty when unsupported) and lane as the library's naming entry points report them
extern "C" int t_fast_select(int kind, int d, int k, int mix_curve, double scale, int screen, int spread, int numpy, int replay,
                             int stats, int batch, int curve_tail, int curve_l2, char *name, int n, int *lane)
{
    gsss::FastAsk a{};
    a.kind = kind;
    a.d = d;
    a.k = k;
    a.mix_curve = mix_curve != 0;
    a.scale = scale;
    a.screen = screen;
    a.spread = spread != 0;
    a.numpy = numpy != 0;
    a.replay = replay != 0;
    a.stats = stats != 0;
    a.batch = batch != 0;
    a.curve_tail = curve_tail;
    a.curve_l2 = curve_l2 != 0;
    gsss::FastPick p;
    const int rc = gsss::fast_select(a, p);
    name[0] = 0;
    *lane = 0;
    if (rc == GSSS_OK) {
        gsss::fast_name(p, name, (size_t)n);
        *lane = p.lane ? 1 : 0;
    }
    return rc;
}
