// Stand-alone driver of hyptokenizer_amd/csrc/hm_gromov_plan.h (tests/test_hyperbolicity_host.py builds it with a host compiler,
// under -fsanitize=address,undefined where the compiler has the runtimes).  For every n of the command line it walks the
// whole tile list, checks it against the double loop it stands for and prints "n nt tiles workspace(n, n) checks-failed";
// then the argument checks over a fixed list of cases, one line each.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../hyptokenizer_amd/csrc/hm_gromov_plan.h"

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; ++a) {
        const int64_t n = atoll(argv[a]);
        const int64_t nt = hm_gr_edge_tiles(n), tiles = hm_gr_tiles(n);
        int64_t t = 0, bad = 0;
        std::vector<char> seen((size_t)tiles, 0);
        for (int64_t ti = 0; ti < nt; ++ti)
            for (int64_t tj = ti; tj < nt; ++tj, ++t) {
                int gi = -1, gj = -1;
                hm_gr_tile_of(nt, t, &gi, &gj);
                if (gi != ti || gj != tj || t >= tiles || seen[(size_t)t]++) ++bad;
                if ((int64_t)gi * HM_GR_TILE >= n || (int64_t)gj * HM_GR_TILE >= n) ++bad;      // every tile holds a pair
            }
        if (t != tiles) ++bad;
        printf("%lld %lld %lld %lld %lld\n", (long long)n, (long long)nt, (long long)tiles, (long long)hm_gr_workspace_bytes(n, n),
               (long long)bad);
    }
    static int x;                                                  // an address that is never dereferenced
    const void* p = &x;
    const struct { const void *d, *base, *val, *wit, *ws; int64_t n, ld, nb; } cases[] = {
        {p, p, p, p, p, 5, 5, 2},          {nullptr, p, p, p, p, 5, 5, 2}, {p, nullptr, p, p, p, 5, 5, 2}, {p, p, nullptr, p, p, 5, 5, 2},
        {p, p, p, nullptr, p, 5, 5, 2},    {p, p, p, p, nullptr, 5, 5, 2}, {p, p, p, p, p, 0, 5, 0},       {p, p, p, p, p, 32769, 40000, 1},
        {p, p, p, p, p, 32768, 32768, 32768}, {p, p, p, p, p, 5, 4, 2},    {p, p, p, p, p, 5, 5, -1},      {p, p, p, p, p, 5, 5, 6},
        {p, p, p, p, p, 5, 9, 0},
    };
    for (const auto& c : cases)
        printf("arg %d %s\n", hm_gr_check_args(c.d, c.n, c.ld, c.base, c.nb, c.val, c.wit, c.ws),
               hm_gr_arg_text(hm_gr_check_args(c.d, c.n, c.ld, c.base, c.nb, c.val, c.wit, c.ws)));
    printf("ws %lld %lld %lld %lld\n", (long long)hm_gr_workspace_bytes(0, 0), (long long)hm_gr_workspace_bytes(5, 6),
           (long long)hm_gr_workspace_bytes(32768, 32768), (long long)hm_gr_workspace_bytes(300, 0));
    return 0;
}
