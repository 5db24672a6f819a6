// hm_timing.h -- the engine's scan timing and statistics with ONE owner, in the style of hm_state.h: the
// fields are private, the searches and the loops say what happened through the named operations below.
//
// Three kinds of timed scan feed the totals (hm_scan_totals), each through add_launch:
//   * a host search reads the engine's own event pair behind its synchronised scan (begin_search / add_pass);
//   * hm_pairwise_argmin_dev leaves the pair unread (note_pending); the next call that cares reads it (flush_pending);
//   * a device-resident loop counts per SEGMENT of its batch (hm_batch_plan.h).  A segment that merged all of its steps is
//     counted -- every scan in the measurement mode of hm_debug_time_loops (read later, read_unread: not inside the call a
//     benchmark is timing), its last scan otherwise.  A segment that stopped early is not counted, whatever it completed.
//     So a call with a redo leaves: in the totals, every complete segment; in hm_last_loop_timing, the last segment when
//     it was complete, zeros otherwise.
// Included by hm_common.h behind the constants (HM_LOOP_MAX_STEPS).
#pragma once

struct HmEvPair { hipEvent_t ev0 = nullptr, ev1 = nullptr; };

class ScanTiming {
public:
    // ---- lifetime (the events carry no system-scope fence around the scan) ----
    hipError_t create()
    {
        const hipError_t st = hipEventCreateWithFlags(&own_.ev0, hipEventDisableSystemFence);
        return st != hipSuccess ? st : hipEventCreateWithFlags(&own_.ev1, hipEventDisableSystemFence);
    }
    // hm_debug_time_loops: an event pair around EVERY scan of a batch segment and one around the segment itself
    hipError_t set_time_loops(bool on)
    {
        for (int q = 0; on && !have_loop_evs_ && q < kLoopEvs; ++q)
            if (!loop_evs_[q])
                if (const hipError_t st = hipEventCreate(&loop_evs_[q]); st != hipSuccess) return st;
        have_loop_evs_ = have_loop_evs_ || on;
        time_loops_ = on;
        return hipSuccess;
    }
    void destroy()
    {
        for (hipEvent_t ev : loop_evs_) if (ev) (void)hipEventDestroy(ev);
        if (own_.ev0) (void)hipEventDestroy(own_.ev0);
        if (own_.ev1) (void)hipEventDestroy(own_.ev1);
    }

    // ---- host searches ----
    HmEvPair own() const { return own_; }                   // the engine's one pair
    void begin_search() { flush_pending(); last_ms_ = 0.f; last_pairs_ = 0; last_emitted_ = 0; last_passes_ = 0; }
    void add_pass(int64_t pairs, int64_t emitted)            // behind a synchronised scan that carried own()
    {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, own_.ev0, own_.ev1);
        last_ms_ += ms; last_passes_ += 1; last_pairs_ = pairs; last_emitted_ = emitted;
        add_launch(ms, pairs);
    }
    void count_pass() { last_passes_ += 1; }                 // a pass that is not timed
    void set_emitted(int64_t emitted) { last_emitted_ = emitted; }
    void note_pending(int64_t pairs) { pending_ = true; pending_pairs_ = pairs; }
    void flush_pending()
    {
        if (!pending_) return;
        pending_ = false;
        if (hipEventSynchronize(own_.ev1) == hipSuccess) read_own(pending_pairs_);
    }

    // ---- device-resident loops, per segment ----
    bool time_all() const { return time_loops_ && have_loop_evs_; }
    void begin_segment() { read_unread(); own_noted_ = false; }          // the loop events are about to be reused
    // the event pair the scan of step k carries (none: nullptrs), with what the scan covers noted for the commit
    hipError_t scan_events(int64_t k, bool is_last, int64_t pairs, hipStream_t s, HmEvPair* ev)
    {
        *ev = HmEvPair();
        if (time_all()) {
            if (k == 0)
                if (const hipError_t st = hipEventRecord(loop_evs_[2 * HM_LOOP_MAX_STEPS], s); st != hipSuccess) return st;
            ev->ev0 = loop_evs_[2 * k]; ev->ev1 = loop_evs_[2 * k + 1];
            pairs_[k] = pairs;
        } else if (is_last) {
            *ev = own_;
            own_noted_ = true; own_pairs_ = pairs;
        }
        return hipSuccess;
    }
    hipError_t end_segment(hipStream_t s) { return time_all() ? hipEventRecord(loop_evs_[2 * HM_LOOP_MAX_STEPS + 1], s) : hipSuccess; }
    // behind the segment's synchronisation
    void commit_segment(int64_t steps, bool complete)
    {
        if (time_all()) {
            batch_ms_ = batch_scan_ms_ = 0.f;
            batch_steps_ = 0;
            if (complete) unread_steps_ = steps;
        } else if (complete && own_noted_) {
            read_own(own_pairs_);
        }
    }
    // the sharded loop's searches run through hm_pairwise_argmin_dev, which asks here for the pair of the step that is open
    hipError_t open_step(int64_t k, int64_t pairs, hipStream_t s) { return time_all() ? scan_events(k, false, pairs, s, &step_) : hipSuccess; }
    void close_step() { step_ = HmEvPair(); }
    HmEvPair step_pair() const { return step_; }
    void read_unread()
    {
        const int64_t steps = unread_steps_;
        if (steps <= 0) return;
        unread_steps_ = 0;
        batch_ms_ = batch_scan_ms_ = 0.f;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, loop_evs_[2 * HM_LOOP_MAX_STEPS], loop_evs_[2 * HM_LOOP_MAX_STEPS + 1]) == hipSuccess) batch_ms_ = ms;
        for (int64_t k = 0; k < steps; ++k) {
            if (hipEventElapsedTime(&ms, loop_evs_[2 * k], loop_evs_[2 * k + 1]) != hipSuccess) continue;
            batch_scan_ms_ += ms;
            add_launch(ms, pairs_[k]);
        }
        batch_steps_ = steps;
    }

    // ---- what the ABI reports ----
    void last_scan(float* ms, int64_t* pairs, int64_t* emitted, int32_t* passes) const
    {
        if (ms) *ms = last_ms_;
        if (pairs) *pairs = last_pairs_;
        if (emitted) *emitted = last_emitted_;
        if (passes) *passes = last_passes_;
    }
    void totals(double* ms, int64_t* pairs, int64_t* launches, bool reset)
    {
        flush_pending();
        read_unread();
        if (ms) *ms = tot_ms_;
        if (pairs) *pairs = tot_pairs_;
        if (launches) *launches = tot_launches_;
        if (reset) { tot_ms_ = 0.0; tot_pairs_ = 0; tot_launches_ = 0; }
    }
    void last_loop(float* batch_ms, float* scan_ms, int64_t* steps)
    {
        read_unread();
        *batch_ms = batch_ms_; *scan_ms = batch_scan_ms_; *steps = batch_steps_;
    }

private:
    void add_launch(float ms, int64_t pairs) { tot_ms_ += ms; tot_pairs_ += pairs; tot_launches_ += 1; }
    // one launch timed by own(): the last search's figures, and the totals count it once (bench: mean launch duration)
    void read_own(int64_t pairs)
    {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, own_.ev0, own_.ev1) != hipSuccess) return;
        last_ms_ = ms; last_pairs_ = pairs; last_passes_ = 1;
        add_launch(ms, pairs);
    }
    static constexpr int kLoopEvs = 2 * HM_LOOP_MAX_STEPS + 2;
    HmEvPair own_, step_;
    bool time_loops_ = false, have_loop_evs_ = false;
    hipEvent_t loop_evs_[kLoopEvs] = {};
    int64_t pairs_[HM_LOOP_MAX_STEPS] = {};                  // pairs behind each timed scan of the current / unread segment
    bool own_noted_ = false, pending_ = false;               // own() rides on this segment's last scan / on an unread argmin_dev scan
    int64_t own_pairs_ = 0, pending_pairs_ = 0;
    float batch_ms_ = 0.f, batch_scan_ms_ = 0.f, last_ms_ = 0.f;
    int64_t batch_steps_ = 0, unread_steps_ = 0, last_pairs_ = 0, last_emitted_ = 0, tot_pairs_ = 0, tot_launches_ = 0;
    int last_passes_ = 0;
    double tot_ms_ = 0.0;
};
