// Stand-alone driver of the three-blocks-per-CU head ring (ring 3 of kScanRings, hyptokenizer_amd/csrc/hm_scan_geom.h) for
// tests/test_scan_ring3_host.py: no HIP, no engine.
//
// "scan_ring3_driver geom": one line per width, ring asked for (1 or 3) and span asked for (1 or 2):
//   "geom KC RING_ASK SPAN_ASK RING SPAN NBUF DIST EXACT TILE_BYTES TILE_LDS SLACK_BYTES LDS_ARGMIN PIECES0 PIECES3"
// "scan_ring3_driver tiles NTILE NBUF SPAN": "tile K FIRST COUNT REQ_FIRST REQ_COUNT OUTSTANDING" per compute tile (ScanRun).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../hyptokenizer_amd/csrc/hm_scan_geom.h"

template <int KC, int RING, int SPAN_ASK>
static void print_geom()
{
    using G = ScanGeom<KC, 1, kScanShapes[0].tm, kScanShapes[0].wpb, HM_SUB_BF16, RING, SPAN_ASK>;
    printf("geom %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", KC, RING, SPAN_ASK, (int)G::RING, (int)G::SPAN, (int)G::NBUF, (int)G::DIST,
           (int)G::EXACT, (int)G::TILE_BYTES, (int)G::TILE_LDS, (int)G::SLACK_BYTES, (int)G::lds_bytes(HM_MODE_ARGMIN), G::wave_pieces(0),
           G::wave_pieces(3));
}
template <int KC>
static void print_width()
{
    print_geom<KC, 1, 1>();
    print_geom<KC, 1, 2>();
    print_geom<KC, 3, 1>();
    print_geom<KC, 3, 2>();
}

// compile-time use, as the kernel's: d = 100 takes the ring, and three of its blocks fit a CU's LDS
static_assert(ScanGeom<13, 1, 2, 4, HM_SUB_BF16, 3, 2>::RING == 3 && ScanGeom<13, 1, 2, 4, HM_SUB_BF16, 3, 2>::lds_bytes(HM_MODE_ARGMIN) == 4 * 13312 + 16, "ring 3 at 13 chunks");
static_assert(ScanRun::outstanding_max(4, 2) == 0, "four slots at span 2: every tile wait is vmcnt(0)");

int main(int argc, char** argv)
{
    const char* what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "geom")) {
        print_width<2>(); print_width<4>(); print_width<8>(); print_width<13>(); print_width<14>(); print_width<16>();
        return 0;
    }
    if (!strcmp(what, "tiles") && argc == 5) {
        const ScanRun run{atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
        if (run.ntile < 0 || run.span < 1 || run.nbuf < 2 * run.span) return 2;
        for (int k = 0; k < run.tiles(); ++k)
            printf("tile %d %d %d %d %d %d\n", k, run.first(k), run.count(k), run.req_first(k), run.req_count(k), run.outstanding(k));
        return 0;
    }
    fprintf(stderr, "usage: scan_ring3_driver geom | tiles NTILE NBUF SPAN\n");
    return 2;
}
