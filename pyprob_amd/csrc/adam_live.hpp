// Live-chunk plan of the Adam pass (host side; plain C++, no device code).
//
// A tensor is TOUCHED once its gradient or its moments may be non-zero: the backward pass marks the tensors its leaves
// write, every other writer of the gradient / moment buffers marks all of them, nothing ever clears a mark. While a tensor
// is untouched its gradient and both moments are exactly zero, so Adam without weight decay is the identity on it: the
// only effect of a step is the tensor's step count. The training paths therefore launch workgroups for the chunks of the
// LIVE tensors only (touched, or weight decay on) - a few contiguous chunk runs whose table travels in the kernel
// arguments - plus one thread per remaining tensor for its step count.
#pragma once
#include <cstdint>
#include <vector>

namespace pp {

constexpr int ADAM_LIVE_MAX_RUNS = 4;      // runs of live chunks the kernel-argument table holds (beyond: the full grid)

struct AdamLiveTable {                     // by-value kernel argument: every index into it is a compile-time constant
    int n_runs;                            // 0: no plan
    int live_blocks;                       // workgroups of all runs; the launch adds one for the tensors between them
    int run_blk[ADAM_LIVE_MAX_RUNS];       // first workgroup of run r
    int run_chunk[ADAM_LIVE_MAX_RUNS];     // first chunk of run r
    int n_gaps;                            // tensor ranges [gap_t0, gap_t1) outside the runs (not live)
    int gap_t0[ADAM_LIVE_MAX_RUNS + 1], gap_t1[ADAM_LIVE_MAX_RUNS + 1];
};

// first[t] = first chunk of tensor t (first[n_tensors] = number of chunks, ascending); live[t] != 0: the tensor is live.
// False: more runs than the table holds (the caller launches the full grid); `tab` is then unspecified.
inline bool adam_live_plan(const int32_t* first, int n_tensors, const uint8_t* live, AdamLiveTable& tab) {
    tab = AdamLiveTable{};
    int blk = 0;
    for (int t = 0; t < n_tensors;) {
        int e = t;
        while (e < n_tensors && (live[e] != 0) == (live[t] != 0)) ++e;
        if (live[t]) {
            if (first[e] > first[t]) {     // (a run of empty tensors launches nothing)
                if (tab.n_runs == ADAM_LIVE_MAX_RUNS) return false;
                tab.run_blk[tab.n_runs] = blk;
                tab.run_chunk[tab.n_runs] = first[t];
                ++tab.n_runs;
                blk += first[e] - first[t];
            }
        } else {
            if (tab.n_gaps == ADAM_LIVE_MAX_RUNS + 1) return false;
            tab.gap_t0[tab.n_gaps] = t;
            tab.gap_t1[tab.n_gaps] = e;
            ++tab.n_gaps;
        }
        t = e;
    }
    tab.live_blocks = blk;
    return true;
}

// Host record of one engine's flat buffers (keyed by the gradient buffer): the tensors' chunk boundaries, the marks and
// the cached table. `version` counts the marks set so far: a table built at a version is valid while it stands.
struct GradTrack {
    const float* grads = nullptr;
    const float* m = nullptr;
    const float* v = nullptr;
    int64_t n_params = 0;
    int n_tensors = 0;
    std::vector<int32_t> first;      // [n_tensors + 1]
    std::vector<uint8_t> touched;    // [n_tensors]
    uint64_t version = 1;
    uint64_t plan_version = 0;       // 0: none cached
    int plan_key = -1;               // weight decay on
    bool plan_ok = false;
    AdamLiveTable plan{};
    uint64_t builds = 0;             // tables built (the tests read it: a steady-state step builds nothing)

    int tensor_of_chunk(int64_t c) const {   // first[t] <= c < first[t + 1]
        int lo = 0, hi = n_tensors;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= c) lo = mid; else hi = mid;
        }
        return lo;
    }
    void touch_tensor(int t) {
        if (!touched[t]) {
            touched[t] = 1;
            ++version;
        }
    }
    void touch_all() {
        for (int t = 0; t < n_tensors; ++t) touch_tensor(t);
    }
    void touch_offset(int64_t off) {         // a float offset into the gradient buffer
        if (off >= 0 && off < n_params && n_tensors > 0) touch_tensor(tensor_of_chunk(off >> 10));
    }
    // the table for this call; false: launch the full grid
    bool table(bool wd_on, const AdamLiveTable** out) {
        const int key = wd_on ? 1 : 0;
        if (plan_version != version || plan_key != key) {
            std::vector<uint8_t> live(touched);
            if (wd_on) live.assign(live.size(), 1);   // weight decay makes a zero gradient a real update
            plan_ok = adam_live_plan(first.data(), n_tensors, live.data(), plan);
            plan_version = version;
            plan_key = key;
            ++builds;
        }
        *out = &plan;
        return plan_ok;
    }
};

}  // namespace pp
