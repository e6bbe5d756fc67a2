// lanes_emul.cpp -- host build of the gate's scheduling policy (opencv-ar_amd/csrc/lanes_core.h) for tests/test_lanes_cpu.py.
// TEST ONLY: nothing in the product links this.
#include "lanes_core.h"

using namespace ocvar;

extern "C" {
int lanes_emul_sizeof() { return (int)sizeof(LaneSched); }
void lanes_emul_init(LaneSched* s, int n_lanes, int width) { lane_sched_init(s, n_lanes, width); }
int lanes_emul_choose(const LaneSched* s) { return lane_choose(s); }
void lanes_emul_book(LaneSched* s, int lane) { lane_book(s, lane); }
void lanes_emul_retire(LaneSched* s, int lane) { lane_retire(s, lane); }
int lanes_emul_outstanding(const LaneSched* s, int lane) { return s->outstanding[lane]; }
long long lanes_emul_wait_for(const LaneSched* s) { return gate_wait_for(s); }
long long lanes_emul_ticket(LaneSched* s) { return gate_ticket(s); }
// lane_of: n ints, the lanes of the in-flight batches (-1: none); done: n ints, non-zero where the simulated clock says finished
static int done_from_table(void* user, int batch) { return static_cast<const int*>(user)[batch]; }
void lanes_emul_refresh(LaneSched* s, int* lane_of, int n, const int* done) {
    int* ptrs[64];
    if (n > 64) n = 64;
    for (int i = 0; i < n; i++) ptrs[i] = lane_of + i;
    lane_refresh(s, ptrs, n, done_from_table, const_cast<int*>(done));
}
int lanes_emul_place(LaneSched* s, int* lane_of, int n, const int* done) {
    int* ptrs[64];
    if (n > 64) n = 64;
    for (int i = 0; i < n; i++) ptrs[i] = lane_of + i;
    return lane_place(s, ptrs, n, done_from_table, const_cast<int*>(done));
}
int lanes_emul_for_queues(int hw_queues, int forced) { return lanes_for_queues(hw_queues, forced); }
int lanes_emul_parse(const char* text) { return parse_queue_count(text); }
int lanes_emul_max() { return LANES_MAX; }
}
