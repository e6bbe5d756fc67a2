// gate.hip -- the gate of include/ocvar_hip.h and its lanes: the streams and events behind lanes_core.h's policy, and the
// contexts' membership.
#include "context.h"
#include <algorithm>
#include <cstdlib>
#include <new>

using namespace ocvar;

// The hardware queues this process runs with are the host's setting: read, never set.
static int lanes_of_this_process(int forced) {
    return lanes_for_queues(parse_queue_count(std::getenv("GPU_MAX_HW_QUEUES")), forced);
}

extern "C" int ocvar_hip_gate_create(OcvarGate** out, int device, int width) { return ocvar_hip_gate_create_lanes(out, device, width, 0); }

extern "C" int ocvar_hip_gate_create_lanes(OcvarGate** out, int device, int width, int lanes) {
    if (!out || width < 1 || width > 64 || lanes < 0 || lanes > LANES_MAX) return OCVAR_E_ARG;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return OCVAR_E_NO_DEVICE;
    OcvarGate* g = new (std::nothrow) OcvarGate();
    if (!g) return OCVAR_E_HIP;
    g->device = device;
    lane_sched_init(&g->sched, lanes_of_this_process(lanes), width);
    g->ring.resize(256);
    bool ok = true;
    // the lanes back to back: the runtime deals streams onto hardware queues in the order they are created
    g->lanes.resize((size_t)g->sched.n_lanes);
    for (auto& l : g->lanes) ok = ok && l.ensure(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : g->ring) ok = ok && e.ensure(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        ocvar_hip_gate_destroy(g);
        return OCVAR_E_HIP;
    }
    *out = g;
    return OCVAR_OK;
}

extern "C" int ocvar_hip_gate_lanes(const OcvarGate* g) { return g ? g->sched.n_lanes : OCVAR_E_ARG; }

// the context's batch no longer counts on its lane (it has been seen complete)
void ocvar::lane_release(OcvarHip* c) {
    OcvarGate* g = c->gate;
    if (!g) return;
    std::lock_guard<std::mutex> lock(g->mu);
    if (c->lane >= 0) lane_retire(&g->sched, c->lane);
    c->lane = -1;
}

// The context leaves its gate.  A batch it has on a lane is waited for first and then belongs to the context's own stream (the
// lane may be destroyed with the gate; a results copy with stream NULL made from here on goes where collect will wait).
void ocvar::gate_detach(OcvarHip* c) {
    OcvarGate* g = c->gate;
    if (!g) return;
    if (c->pending && c->on_lane) {
        (void)batch_wait(c);
        c->on_lane = false;
        c->copy_pending = false;
        c->last_stream = c->stream;
    }
    lane_release(c);
    {
        std::lock_guard<std::mutex> lock(g->mu);
        auto& a = g->attached;
        a.erase(std::remove(a.begin(), a.end(), c), a.end());
    }
    c->gate = nullptr;
}

extern "C" void ocvar_hip_gate_destroy(OcvarGate* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    for (auto& l : g->lanes)   // (a batch of a context that is still attached may be on a lane)
        if (l) (void)hipStreamSynchronize(l);
    while (!g->attached.empty()) gate_detach(g->attached.back());
    delete g;
}

extern "C" int ocvar_hip_set_gate(OcvarHip* c, OcvarGate* g) {
    if (!c || (g && g->device != c->device)) return OCVAR_E_ARG;
    if (g == c->gate) return OCVAR_OK;
    (void)hipSetDevice(c->device);
    gate_detach(c);   // (waits for a batch on a lane of the old gate; it is collected as usual)
    c->gate = g;
    if (g) {
        std::lock_guard<std::mutex> lock(g->mu);
        g->attached.push_back(c);
    }
    return OCVAR_OK;
}

// The lane for the next batch of a context of the gate (lanes_core.h: lane_place), booked.  "Finished" is a query of the
// batch's last event.
static int lane_batch_done(void* user, int i) {
    OcvarHip* o = (*static_cast<std::vector<OcvarHip*>*>(user))[(size_t)i];
    if (hipEventQuery(o->ev[EV_LAST]) == hipSuccess) return 1;
    (void)hipGetLastError();   // (not ready: no error)
    return 0;
}
int ocvar::gate_place(OcvarGate* g) {
    std::lock_guard<std::mutex> lock(g->mu);
    int* lane_of[64];
    const int n = (int)std::min<size_t>(g->attached.size(), 64);
    for (int i = 0; i < n; i++) lane_of[i] = &g->attached[(size_t)i]->lane;
    return lane_place(&g->sched, lane_of, n, lane_batch_done, &g->attached);
}

// before / after a gated launch on stream s: the ticket is taken once the launch and its event are in the stream
hipError_t ocvar::gate_enter(OcvarGate* g, hipStream_t s) {
    if (!g) return hipSuccess;
    const long long wait_for = gate_wait_for(&g->sched);
    if (wait_for < 0) return hipSuccess;
    return hipStreamWaitEvent(s, g->ring[(size_t)wait_for % g->ring.size()], 0);
}
hipError_t ocvar::gate_leave(OcvarGate* g, hipStream_t s) {
    if (!g) return hipSuccess;
    const hipError_t e = hipEventRecord(g->ring[(size_t)g->sched.issued % g->ring.size()], s);
    (void)gate_ticket(&g->sched);
    return e;
}
