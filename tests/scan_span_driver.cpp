// Stand-alone driver of the ring walk's decomposition (ScanRun and ScanGeom::SPAN of hyptokenizer_amd/csrc/hm_scan_geom.h:
// the code the head kernels run) for tests/test_scan_span_host.py and tests/test_scan_head_span.py: no HIP, no engine.
//
// "scan_span_driver check": walks a ring through every run of 0 .. 70 slots, both spans, both ring depths and both widths
// with a head test, and checks what the kernel relies on; prints "ok CASES" or the first violation (exit status 1).
// "scan_span_driver geom": "geom KC RING SPAN_ASK SPAN NBUF DIST PIECES_MAX" per width, ring and span asked for.
// "scan_span_driver tiles NTILE NBUF SPAN": "tile K FIRST COUNT REQ_FIRST REQ_COUNT OUTSTANDING" per compute tile.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../hyptokenizer_amd/csrc/hm_scan_geom.h"

#define FAIL(...) do { printf("FAIL ntile %d nbuf %d span %d tile %d: ", run.ntile, run.nbuf, run.span, k); printf(__VA_ARGS__); printf("\n"); return false; } while (0)

// one run through a ring of nbuf slots; `dist`: the ring's depth, `pieces`: the most 1 KiB pieces a wave moves per slot
static bool walk(const ScanRun run, int dist, int pieces)
{
    int k = -1;
    std::vector<int> holds(run.nbuf, -1);      // the run's slot a ring slot holds (requested or landed), -1: nothing yet
    int requested = 0, landed = 0, computed = 0;   // slots [0, requested) are requested, [0, landed) have landed, [0, computed) are computed
    auto request = [&](int first, int count, int reading_first, int reading_count) {
        for (int s = first; s < first + count; ++s) {
            if (s != requested) return false;                                   // in order, none twice, none left out
            const int b = s % run.nbuf;
            if (holds[b] >= reading_first && holds[b] < reading_first + reading_count) return false;   // a tile still reads it
            if (holds[b] >= computed) return false;                             // it holds a slot nobody has computed yet
            holds[b] = s;
            ++requested;
        }
        return true;
    };
    if (run.nbuf < 2 * run.span) FAIL("ring too small for the span");
    if (!request(0, run.prologue(), 0, 0)) FAIL("prologue");
    landed = requested;
    if (run.prologue() != (run.ntile < run.nbuf - run.span ? run.ntile : run.nbuf - run.span)) FAIL("prologue count");
    for (k = 0; k < run.tiles(); ++k) {
        const int first = run.first(k), count = run.count(k);
        if (count < 1 || count > run.span) FAIL("a tile of %d slots", count);
        if (count < run.span && k != run.tiles() - 1) FAIL("a short tile in mid-run");
        const int before = requested;
        // the slots of tile k - 1 are free (every wave is behind the barrier that ended it); tile k's are being read
        if (first != computed) FAIL("computes slot %d, next is %d", first, computed);
        if (!request(run.req_first(k), run.req_count(k), first, count)) FAIL("request of %d slots from %d", run.req_count(k), run.req_first(k));
        if (run.req_count(k) == 0 && requested < run.ntile) FAIL("nothing requested with %d slots to go", run.ntile - requested);
        for (int s = first; s < first + count; ++s) {
            if (s >= landed) FAIL("slot %d computed before it landed", s);
            if (holds[s % run.nbuf] != s) FAIL("slot %d is no longer in the ring", s);
        }
        computed += count;
        const int out = run.outstanding(k);
        if (out < 0) FAIL("%d outstanding", out);            // (more than is in flight -- the prologue's slots have all landed -- is a wait that passes)
        if (out > dist - run.span) FAIL("%d outstanding, more than DIST - span", out);
        if (out > ScanRun::outstanding_max(run.nbuf, run.span)) FAIL("%d outstanding, more than the waits are written for", out);
        if (out * pieces > 60) FAIL("%d pieces do not fit vmcnt", out * pieces);
        // span 2 picks the tile's key load up behind the tile's own wait (span 1: DIST - 1 tiles later): whatever that wait
        // leaves in flight must have been requested behind the load, in this tile
        const int flying = landed > requested - out ? landed : requested - out;
        if (run.span > 1 && flying < requested && flying < before) FAIL("the wait leaves slot %d of an earlier tile in flight: it need not have passed the key load", flying);
        if (requested - out > landed) landed = requested - out;
        if (k + 1 < run.tiles() && landed < run.first(k + 1) + run.count(k + 1)) FAIL("the next tile's slots have not landed");
        if (k == run.tiles() - 1 && out != 0) FAIL("the run's last wait leaves something in flight");
    }
    if (computed != run.ntile || requested != run.ntile || landed != run.ntile) FAIL("run ends with %d computed, %d requested, %d landed", computed, requested, landed);
    return true;
}

template <int KC, int RING, int SPAN_ASK>
static bool check_geom(bool print, int* cases)
{
    using G = ScanGeom<KC, 1, kScanShapes[0].tm, kScanShapes[0].wpb, HM_SUB_BF16, RING, SPAN_ASK>;
    const int pieces = G::wave_pieces(0);
    if (print) { printf("geom %d %d %d %d %d %d %d\n", KC, RING, SPAN_ASK, (int)G::SPAN, (int)G::NBUF, (int)G::DIST, pieces); return true; }
    for (int ntile = 0; ntile <= 70; ++ntile, ++*cases)
        if (!walk(ScanRun{ntile, G::NBUF, G::SPAN}, G::DIST, pieces)) return false;
    return true;
}
template <int KC>
static bool check_width(bool print, int* cases)
{
    return check_geom<KC, 1, 1>(print, cases) && check_geom<KC, 1, 2>(print, cases) && check_geom<KC, 2, 1>(print, cases) && check_geom<KC, 2, 2>(print, cases);
}

// compile-time use, as the kernel's: a run of 7 slots over 5 ring slots in tiles of two ends on a tile of one
static_assert(ScanRun{7, 5, 2}.tiles() == 4 && ScanRun{7, 5, 2}.count(3) == 1 && ScanRun{7, 5, 2}.outstanding(0) == 1 && ScanRun{7, 5, 2}.outstanding(3) == 0, "ScanRun is constexpr");

int main(int argc, char** argv)
{
    const char* what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "check") || !strcmp(what, "geom")) {
        const bool print = what[0] == 'g';
        int cases = 0;
        // the widths of the bf16 form whose rows have a head test (8 chunks on: d = 50 .. 128)
        if (!(check_width<8>(print, &cases) && check_width<13>(print, &cases) && check_width<14>(print, &cases) && check_width<16>(print, &cases))) return 1;
        if (!print) printf("ok %d\n", cases);
        return 0;
    }
    if (!strcmp(what, "tiles") && argc == 5) {
        const ScanRun run{atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
        if (run.ntile < 0 || run.span < 1 || run.nbuf < 2 * run.span) return 2;
        for (int k = 0; k < run.tiles(); ++k)
            printf("tile %d %d %d %d %d %d\n", k, run.first(k), run.count(k), run.req_first(k), run.req_count(k), run.outstanding(k));
        return 0;
    }
    fprintf(stderr, "usage: scan_span_driver check | geom | tiles NTILE NBUF SPAN\n");
    return 2;
}
