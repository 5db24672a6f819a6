// hm_batch_plan.h -- which steps of a standard-loop batch are issued next, and in which form.  Plain host
// C++, no HIP: the driver (hm_std_merge_steps, hm_loops.hip) issues the segment the plan names, reports how many of its
// leading steps merged and the loop's stop word, and asks again.  No recursion, no allocation; at most 2 * steps + 1
// segments (every redo of a single step is followed by at least that one merged step).
//
//   last segment       outcome                     next
//   (start)                                        [0, steps), may pipeline
//   any                all `count` merged          done
//   sequential         fewer merged                done (the batch ends at that record)
//   pipelined          stop 5 (order guard)        [first + merged, steps), sequential; no pipelining for the rest of the call
//   pipelined          stop 6 (tail overflow)      [first + merged, +1), sequential: that ONE step through the full-size tail
//   that single step   merged, steps remain        [.., steps), may pipeline again (and may meet 6 again)
//   that single step   did not merge (found 0, 2)  done
//   pipelined          stop 1 or 2                 done
#pragma once
#include <stdint.h>

struct BatchSegment {
    int64_t first_step, count;
    bool may_pipeline;          // the driver still decides by the table as it stands then
};

class BatchPlan {
public:
    explicit BatchPlan(int64_t steps) : steps_(steps), seg_{0, steps, true}, pending_(steps > 0) {}

    bool pending() const { return pending_; }
    const BatchSegment& segment() const { return seg_; }
    int64_t done() const { return done_; }                  // leading steps of the batch that merged
    // the search state is armed after the call iff the last segment was sequential and merged all of its steps (a
    // pipelined segment leaves its two sets armed for ITS next steps only)
    bool leaves_armed() const { return armed_; }

    // the pending segment was issued: pipelined or not, `merged` leading steps merged, the loop's stop word
    void report(bool pipelined, int64_t merged, uint32_t stop)
    {
        const bool complete = merged == seg_.count, was_single = single_;
        done_ = seg_.first_step + merged;
        armed_ = !pipelined && complete;
        single_ = false;
        pending_ = false;
        if (complete) {
            if (was_single && done_ < steps_) next(steps_ - done_, may_pipeline_);
        } else if (pipelined && stop == 5u) {
            may_pipeline_ = false;
            next(steps_ - done_, false);
        } else if (pipelined && stop == 6u) {
            single_ = true;
            next(1, false);
        }
    }

private:
    void next(int64_t count, bool may_pipeline)
    {
        seg_.first_step = done_; seg_.count = count; seg_.may_pipeline = may_pipeline;
        pending_ = true;
    }
    int64_t steps_, done_ = 0;
    BatchSegment seg_;
    bool pending_, may_pipeline_ = true, single_ = false, armed_ = false;
};
