// hm_state.h -- the search state that hm_engine carries from one call to the next, with ONE owner:
// the fields are private, reads go through const accessors and writes only through the named transitions below, so an
// entry point says which transition it is ("an existing row changed") instead of spelling out which fields that voids.
// Plain host C++: what lives on the device beside it (the argmin seed d_seed, the previous list d_prev, the norm bounds)
// stays with the engine; where a transition also has to zero the seed, hm_rows_changed (hm_engine.hip) pairs the two.
#pragma once
#include <stdint.h>

class SearchState {
public:
    // emission cut predicted from the previous whole-table top-k: valid while rows are only appended
    struct Cut {
        bool have = false;
        uint32_t bits = 0;      // largest u' of that selection
        int64_t k = 0;
        float c = 0.f;
        bool debug = false;     // hm_debug_force_cut: the next top-k that uses the cut starts from `bits` as given
    };
    // the ordered list of the last whole-table top-k (hm_engine::d_prev holds the entries)
    struct Prev {
        bool valid = false;
        int64_t k = 0, n = 0;
        float thr = 0.f;
    };
    // hm_topk_refresh_begin .. _end
    struct Refresh {
        bool pending = false;
        int64_t k = 0;
        float c = 0.f, thr = 0.f;
        void* stream = nullptr;
    };

    const Cut& cut() const { return cut_; }
    const Prev& prev() const { return prev_; }
    const Refresh& refresh() const { return refresh_; }

    // ---- arming: counters and running key left on the device, ready for the next argmin of the same range ----
    // An argmin of (rb, re) starts: true = its predecessor armed this very range (no seed-init launch).  Disarms either way.
    bool take_arm(int64_t rb, int64_t re)
    {
        const bool same = armed_ && armed_rb_ == rb && armed_re_ == re;
        armed_ = false;
        return same;
    }
    void arm(int64_t rb, int64_t re) { armed_ = true; armed_rb_ = rb; armed_re_ = re; }
    void disarm() { armed_ = false; }          // any other search, any knob

    // ---- voiding ----
    // an existing row changed: arming and cut are void (so is the device seed: hm_rows_changed)
    void row_changed() { armed_ = false; cut_.have = false; }
    // the table was replaced or its form changed: also forget which route its searches took.  (The previous list is
    // switched off through the cut.)
    void table_replaced()
    {
        row_changed();
        f32_thr_ = 0.0f;
        exact_thr_ = 0.0f;
    }

    // ---- cut and previous list ----
    // a top-k search delivered its list.  keep: it was a whole-table search that filled k -- `bits` (the largest u' of the
    // selection) is a guaranteed superset cut for the next refresh while rows are only appended.  Otherwise both are dropped.
    void publish(bool keep, uint32_t bits, int64_t k, float c, int64_t n, float thr)
    {
        if (!keep) return drop_list();
        cut_.have = true; cut_.bits = bits; cut_.k = k; cut_.c = c;
        prev_.valid = true; prev_.k = k; prev_.n = n; prev_.thr = thr;
    }
    void drop_prev() { prev_.valid = false; }                       // a top-k that selected nothing: the cut stays
    void drop_list() { cut_.have = false; prev_.valid = false; }    // range searches do not feed the whole-table refresh
    // hm_pairwise_count searches without the cut and leaves it as it found it
    Cut suspend_cut()
    {
        const Cut saved = cut_;
        cut_.have = false;
        return saved;
    }
    void restore_cut(const Cut& saved) { cut_.have = saved.have; cut_.bits = saved.bits; cut_.k = saved.k; cut_.c = saved.c; }
    void force_cut(uint32_t bits, int64_t k, float c) { cut_.have = true; cut_.bits = bits; cut_.k = k; cut_.c = c; cut_.debug = true; }
    bool consume_debug_cut()
    {
        const bool was = cut_.debug;
        cut_.debug = false;
        return was;
    }
    // when the k smallest of a table of n rows are the k smallest of (the previous list) + (the pairs of the rows appended since)
    bool incremental_ok(int64_t n, float c, float thr, int64_t k) const
    {
        return k > 0 && cut_.have && prev_.valid && prev_.k == k && cut_.c == c && thr >= prev_.thr && n >= prev_.n &&
               n - prev_.n <= 8192 && cut_.bits > 0x3f800000u && !cut_.debug;
    }

    // ---- route memories, per table: from this threshold on a search goes straight to the fp32 prefilter / the exact path ----
    bool straight_to_f32(float thr) const { return f32_thr_ > 0.0f && thr >= f32_thr_; }
    bool straight_to_exact(float thr) const { return exact_thr_ > 0.0f && thr >= exact_thr_; }
    void remember_f32(float thr) { if (!(f32_thr_ > 0.0f && f32_thr_ <= thr)) f32_thr_ = thr; }
    void remember_exact(float thr) { if (!(exact_thr_ > 0.0f && exact_thr_ <= thr)) exact_thr_ = thr; }

    // ---- the refresh in two halves ----
    void refresh_begin(int64_t k, float c, float thr, void* stream)
    {
        refresh_.pending = true;
        refresh_.k = k; refresh_.c = c; refresh_.thr = thr; refresh_.stream = stream;
    }
    void refresh_end() { refresh_.pending = false; }

private:
    bool armed_ = false;
    int64_t armed_rb_ = 0, armed_re_ = 0;
    Cut cut_;
    Prev prev_;
    Refresh refresh_;
    float f32_thr_ = 0.0f, exact_thr_ = 0.0f;
};
