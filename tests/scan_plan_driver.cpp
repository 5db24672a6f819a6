// Stand-alone driver of the pair scan's host policy (hyptokenizer_amd/csrc/hm_scan_plan.h, hm_scan_geom.h) for
// tests/test_scan_plan.py: no HIP, no engine.
//
// "scan_plan_driver geom": text on stdout --
//   "ng W..." / "kc W..."                 the instantiated widths, as the engine's tables list them
//   "shape S TM WPB ROWS"                 the block shapes
//   "geom NG BF TM WPB SUB MODE LDS NTHREADS BLOCK_ROWS"   ScanGeom of every (width, shape, mode) the dispatch can instantiate
//
// "scan_plan_driver plan": stdin, one line per case --
//   chunk_f32 chunk_bf16 tail_fraction tail_div phases share0..4 div0..5 force_shape big_min_rows
//   n row_begin row_end n_limit col_begin bf16 KC
// stdout, binary int32: per case the plan -- ok, n, row_begin, row_end, col_begin, shape, rb_first, nct, n_items, n_ph,
// items[6], rb0[6], chunks[6], ch[6], ctmin[6] -- and, when ok, (rb, ct0, ct1) of every item 0 .. n_items - 1 as hm_scan_item
// decodes it for that shape's rows per block.
#include <stdio.h>

#include <vector>

#include "../hyptokenizer_amd/csrc/hm_scan_plan.h"

template <int NG, int BF, int S, int SUB>
static void geom_line()
{
    using G = ScanGeom<NG, BF, kScanShapes[S].tm, kScanShapes[S].wpb, SUB>;
    for (int mode = HM_MODE_TOPK; mode <= HM_MODE_HIST; ++mode)
        printf("geom %d %d %d %d %d %d %d %d %d\n", NG, BF, kScanShapes[S].tm, kScanShapes[S].wpb, SUB, mode, G::lds_bytes(mode), (int)G::NTHREADS,
               (int)G::BLOCK_ROWS);
}
template <int KC>
static void geom_bf16()
{
    geom_line<KC, 1, 0, HM_SUB_BF16>();
    if constexpr (KC <= HM_SCAN_BIG_MAX_KC) {
        geom_line<KC, 1, 1, HM_SUB_BF16>();
        geom_line<KC, 1, 2, HM_SUB_BF16>();
        geom_line<KC, 1, 3, HM_SUB_BF16>();
        geom_line<KC, 1, 4, HM_SUB_BF16>();
    }
}

static int geom()
{
#define W(v) printf(" %d", v);
    printf("ng"); HM_SCAN_NG_LIST(W, HM_SCAN_WIDTHS_ALL) printf("\n");
    printf("kc"); HM_SCAN_KC_LIST(W, HM_SCAN_WIDTHS_ALL) printf("\n");
#undef W
    for (int s = 0; s < HM_SCAN_SHAPES; ++s) printf("shape %d %d %d %d\n", s, kScanShapes[s].tm, kScanShapes[s].wpb, hm_shape_rows(s));
#define NG_GEOM(v) geom_line<v, 0, 0, HM_SUB_F32>();
#define KC_GEOM(v) geom_bf16<v>();
    HM_SCAN_NG_LIST(NG_GEOM, HM_SCAN_WIDTHS_ALL)
    HM_SCAN_KC_LIST(KC_GEOM, HM_SCAN_WIDTHS_ALL)
#undef NG_GEOM
#undef KC_GEOM
    return 0;
}

static int plans()
{
    ScanPlanKnobs k;
    ScanRequest rq;
    long long big = 0, v[5];
    std::vector<int> out;
    for (;;) {
        int got = scanf(" %d %d %lf %d %d", &k.chunk_f32, &k.chunk_bf16, &k.tail_fraction, &k.tail_div, &k.phases);
        if (got == EOF) break;
        if (got != 5) return 1;
        for (int q = 0; q < HM_SCAN_PHASES - 1; ++q) if (scanf(" %lf", &k.ph_share[q]) != 1) return 1;
        for (int q = 0; q < HM_SCAN_PHASES; ++q) if (scanf(" %d", &k.ph_div[q]) != 1) return 1;
        if (scanf(" %d %lld %lld %lld %lld %lld %lld %d %d", &k.force_shape, &big, &v[0], &v[1], &v[2], &v[3], &v[4], &rq.bf16, &rq.KC) != 9) return 1;
        k.big_min_rows = big;
        rq.n = v[0]; rq.row_begin = v[1]; rq.row_end = v[2]; rq.n_limit = v[3]; rq.col_begin = v[4];
        const ScanPlan pl = hm_scan_plan(k, rq);
        out.assign({pl.ok ? 1 : 0, pl.n, pl.row_begin, pl.row_end, pl.col_begin, pl.shape, pl.rb_first, pl.nct, pl.n_items, pl.items.n_ph});
        for (const int* a : {pl.items.items, pl.items.rb0, pl.items.chunks, pl.items.ch, pl.items.ctmin}) out.insert(out.end(), a, a + HM_SCAN_PHASES);
        if (pl.ok) {
            const int block_rows = hm_shape_rows(pl.shape), cols = 32 * (rq.bf16 ? HM_SUB_BF16 : HM_SUB_F32);
            for (int item = 0; item < pl.n_items; ++item) {
                int rb = 0, ct0 = 0, ct1 = 0;
                hm_scan_item(pl.items, item, block_rows, cols, pl.nct, pl.col_begin, &rb, &ct0, &ct1);
                out.insert(out.end(), {rb, ct0, ct1});
            }
        }
        if (fwrite(out.data(), sizeof(int), out.size(), stdout) != out.size()) return 1;
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && argv[1][0] == 'g') return geom();
    if (argc == 2 && argv[1][0] == 'p') return plans();
    fprintf(stderr, "usage: scan_plan_driver geom | plan\n");
    return 2;
}
