// lanes_core.h -- the gate's scheduling policy, free of HIP calls (gate.hip drives it with streams and events, tests/emul with a
// simulated timeline): how many lanes a gate opens, which lane a batch goes to, and the tickets of the gated launches.
//
// A lane is a stream the gate owns.  The runtime deals streams onto the process's hardware queues, and streams that share a
// queue run one after the other -- a wait in front of one context's kernels also holds back whatever another context put
// behind it in that queue.  With one stream per context and fewer queues than contexts the same contexts share a queue for
// ever.  The gate therefore opens one lane per queue and places every batch, when it is enqueued, on the lane with the least
// outstanding work: the doubled-up lane rotates, and the batch queued behind another is what keeps a lane busy while the host
// collects and re-enqueues.
#pragma once

namespace ocvar {

constexpr int LANES_MAX = 8;          // more streams than this buy nothing: five contexts fill the GPU
constexpr int HW_QUEUES_DEFAULT = 4;  // what the HIP runtime opens when GPU_MAX_HW_QUEUES is not set

// Lanes for a process that runs with `hw_queues` hardware queues (the value of GPU_MAX_HW_QUEUES, <= 0: not set): one per
// queue.  Created back to back before the contexts' own streams they land on distinct queues, the null stream's included
// (kernel trace of bench.py at four queues: four lanes on queues 1 - 4, 250 k frames/s; three lanes, one queue left to the
// null stream: 225 k).  forced > 0 overrides (experiments, tests).
inline int lanes_for_queues(int hw_queues, int forced) {
    int n = forced > 0 ? forced : (hw_queues > 0 ? hw_queues : HW_QUEUES_DEFAULT);
    return n < 1 ? 1 : (n > LANES_MAX ? LANES_MAX : n);
}

// the decimal value of an environment variable, 0 when absent or not a positive number
inline int parse_queue_count(const char* text) {
    if (!text) return 0;
    long v = 0;
    for (const char* p = text; *p; p++) {
        if (*p < '0' || *p > '9') return 0;
        v = v * 10 + (*p - '0');
        if (v > 1 << 20) return 0;
    }
    return (int)v;
}

struct LaneSched {
    int n_lanes = 1;
    int width = 1;                                  // gated launches that may run at once
    int outstanding[LANES_MAX] = {};                // batches placed on the lane and not yet retired
    unsigned long long newest[LANES_MAX] = {};      // sequence number of the lane's newest batch (0: never used)
    unsigned long long placed = 0;                  // batches placed so far
    unsigned long long issued = 0;                  // tickets handed out so far
};

inline void lane_sched_init(LaneSched* s, int n_lanes, int width) {
    *s = LaneSched();
    s->n_lanes = n_lanes < 1 ? 1 : (n_lanes > LANES_MAX ? LANES_MAX : n_lanes);
    s->width = width < 1 ? 1 : width;
}

// The lane of the next batch: least outstanding work, ties to the lane whose newest batch is oldest (it drains first).
inline int lane_choose(const LaneSched* s) {
    int best = 0;
    for (int l = 1; l < s->n_lanes; l++)
        if (s->outstanding[l] < s->outstanding[best] ||
            (s->outstanding[l] == s->outstanding[best] && s->newest[l] < s->newest[best]))
            best = l;
    return best;
}

inline void lane_book(LaneSched* s, int lane) {
    s->outstanding[lane]++;
    s->newest[lane] = ++s->placed;
}

// a batch of the lane has been seen complete (collected, or its last event queried)
inline void lane_retire(LaneSched* s, int lane) {
    if (lane >= 0 && lane < s->n_lanes && s->outstanding[lane] > 0) s->outstanding[lane]--;
}

// Brings the lanes up to date before a placement: a batch that has finished on the device but has not been collected yet is
// no outstanding work.  *lane_of[i] is the lane that still counts in-flight batch i (-1: none); done(user, i) says whether
// that batch has finished (gate.hip: a query of its last event; the tests: a simulated clock).
typedef int (*LaneDoneFn)(void* user, int batch);
inline void lane_refresh(LaneSched* s, int* const* lane_of, int n, LaneDoneFn done, void* user) {
    for (int i = 0; i < n; i++)
        if (*lane_of[i] >= 0 && done(user, i)) {
            lane_retire(s, *lane_of[i]);
            *lane_of[i] = -1;
        }
}

// The whole placement of a batch: refresh, choose, book.
inline int lane_place(LaneSched* s, int* const* lane_of, int n, LaneDoneFn done, void* user) {
    lane_refresh(s, lane_of, n, done, user);
    const int lane = lane_choose(s);
    lane_book(s, lane);
    return lane;
}

// Tickets of the gated launches, in the order the host issues them: launch n may start when launch n - width has finished.
// gate_wait_for: the ticket the next launch has to wait for, -1 for the first `width` launches; gate_ticket: the next launch's
// own ticket, handed out once the launch is in its stream (a launch that failed to get there takes none).  The launch a
// ticket waits for was issued earlier, and so was everything in front of that launch in its lane: the waits cannot form a
// cycle, whatever the number of lanes and contexts.
inline long long gate_wait_for(const LaneSched* s) {
    const long long w = (long long)s->issued - s->width;
    return w < 0 ? -1 : w;
}
inline long long gate_ticket(LaneSched* s) { return (long long)s->issued++; }

}  // namespace ocvar
