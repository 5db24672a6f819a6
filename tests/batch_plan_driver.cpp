// Stand-alone driver of BatchPlan (hyptokenizer_amd/csrc/hm_batch_plan.h) for tests/test_batch_plan.py: no HIP, no engine.
// stdin:  per case a line "case STEPS", then one line "PIPELINED MERGED STOP" per segment the plan is expected to issue.
// stdout: per case "case STEPS", one line "seg FIRST COUNT MAY_PIPELINE" per segment issued, then
//         "end DONE ARMED" -- or "starved" / "runaway" / "bad" when the plan and the script part ways.
#include <stdio.h>

#include "../hyptokenizer_amd/csrc/hm_batch_plan.h"

int main()
{
    long long steps = 0;
    while (scanf(" case %lld", &steps) == 1) {
        printf("case %lld\n", steps);
        BatchPlan plan(steps);
        long long issued = 0;
        const char* verdict = nullptr;
        while (plan.pending() && !verdict) {
            const BatchSegment seg = plan.segment();
            printf("seg %lld %lld %d\n", (long long)seg.first_step, (long long)seg.count, seg.may_pipeline ? 1 : 0);
            int pipelined = 0;
            long long merged = 0;
            unsigned stop = 0;
            if (++issued > 2 * steps + 1) verdict = "runaway";
            else if (scanf(" %d %lld %u", &pipelined, &merged, &stop) != 3) verdict = "starved";
            else if ((pipelined && !seg.may_pipeline) || merged < 0 || merged > seg.count) verdict = "bad";
            else plan.report(pipelined != 0, merged, stop);
        }
        if (verdict) { printf("%s\n", verdict); return 1; }
        printf("end %lld %d\n", (long long)plan.done(), plan.leaves_armed() ? 1 : 0);
    }
    return 0;
}
