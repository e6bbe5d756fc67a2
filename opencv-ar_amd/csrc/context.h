// context.h -- private to the host files of the C ABI (api.hip, frame_ops.hip, gate.hip, host_transport.hip, debug.hip): the
// context and the gate, the owners of their HIP resources, the fence of a workspace shared by calls on any stream, and the few
// functions those files share.
#pragma once
#include "kernels.h"
#include "lanes_core.h"
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

namespace ocvar {

// One owner per HIP resource: what a context or a gate holds is released when it is deleted, whichever call created it and
// however far its creation got.  Move-only; each converts to the handle or pointer it owns.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t ensure(unsigned flags) { return s ? hipSuccess : hipStreamCreateWithFlags(&s, flags); }   // created on first use
    operator hipStream_t() const { return s; }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t ensure(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }   // created on first use
    operator hipEvent_t() const { return e; }
};

// Orders the uses of a workspace shared by calls on any stream: a use lies between enter(s) and leave(s), and waits (on its
// stream) for the last one when that ran on another stream.  drain(): the host waits for the last use, before the workspace or
// what its kernels read is freed or rewritten.
struct WorkspaceFence {
    Event done;                  // behind the last use, on `last` (created on first use)
    hipStream_t last = nullptr;
    bool used = false;
    hipError_t enter(hipStream_t s) {
        const hipError_t e = done.ensure(hipEventDisableTiming);
        return e == hipSuccess && used && last != s ? hipStreamWaitEvent(s, done, 0) : e;
    }
    hipError_t leave(hipStream_t s) {
        const hipError_t e = hipEventRecord(done, s);
        if (e == hipSuccess) last = s, used = true;
        return e;
    }
    hipError_t drain() const { return used ? hipEventSynchronize(done) : hipSuccess; }
};

// Device memory, or page-locked host memory, that grows on demand: reserve(n) leaves at least n bytes -- a larger request
// frees the block and allocates a new one (the contents are not kept); on failure the buffer is empty, size 0.
template <typename T, bool PINNED>
struct Buffer {
    T* p = nullptr;
    size_t bytes = 0;
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    ~Buffer() { (void)release(); }
    hipError_t release() {
        const hipError_t e = !p ? hipSuccess : (PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr, bytes = 0;
        return e;
    }
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        hipError_t e = release();
        void* q = nullptr;
        if (e == hipSuccess) e = PINNED ? hipHostMalloc(&q, n) : hipMalloc(&q, n);
        if (e != hipSuccess) return e;
        p = static_cast<T*>(q);
        bytes = n;
        return hipSuccess;
    }
    operator T*() const { return p; }
};
template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

// The events of a batch: ev[0] in front of the first kernel, ev[k] between stage k and stage k + 1, ev[EV_LAST] behind the
// batch's last copy -- what collect waits for and what work that follows the batch is ordered behind.  ocvar_hip_stage_ms
// reports the EV_STAGES intervals ev[k] .. ev[k + 1] one by one, then the whole batch ev[0] .. ev[EV_LAST].
constexpr int EV_COUNT = 13, EV_LAST = EV_COUNT - 1, EV_STAGES = EV_LAST - 1;
// ocvar_hip_set_tuning's knobs are 1 .. TUNE_KNOBS - 1 (OCVAR_TUNE_*)
constexpr int TUNE_KNOBS = OCVAR_TUNE_BAYER_PAIRS + 1;

}  // namespace ocvar

struct OcvarHip;

// At most `width` binarise kernels of the contexts that share the gate run at once: launch n waits (on its stream) for the
// event recorded behind launch n - width.  The gate also owns the lanes: the streams on which the batches of its contexts run
// when the caller names none (lanes_core.h has the policy; here are the streams, the events and the contexts' bookkeeping).
struct OcvarGate {
    int device = 0;
    std::mutex mu;                  // the lanes' bookkeeping: contexts may be collected and destroyed from other threads than the
                                    // one that enqueues (sched's lane counts, `attached`, the contexts' `lane`)
    ocvar::LaneSched sched;         // placement of batches on lanes, tickets of the gated launches
    std::vector<ocvar::Event> ring;     // far more slots than launches can be in flight (contexts x 2)
    std::vector<ocvar::Stream> lanes;   // (destroyed before the ring's events)
    std::vector<OcvarHip*> attached;    // the contexts that have this gate (ocvar_hip_set_gate)
};

// (The streams are declared first, then the events, then the memory: a context's memory is freed first, its streams last.)
struct OcvarHip {
    int device = 0;
    OcvarGate* gate = nullptr;
    int result_limit = OCVAR_MAX_MARKERS;   // marker records per frame copied to the host (ocvar_hip_set_result_limit)
    int input_format = OCVAR_FMT_BGR;       // what the frames of the next batch hold (ocvar_hip_set_input_format)
    ocvar::RefineArgs refine{};             // corner refinement of the next batch (ocvar_hip_set_corner_refine): half_win 0 = off
    int tune[ocvar::TUNE_KNOBS] = {};       // ocvar_hip_set_tuning: 0 = default
    ocvar::Workspace ws{};
    ocvar::Stream stream;
    ocvar::Stream hp_stream;           // high-priority stream for the kernels OCVAR_TUNE_HP_MASK names (created on first use)
    ocvar::Stream h2d_stream, d2h_stream;   // host transport of ocvar_hip_detect_host (created on first use)
    hipStream_t last_stream = nullptr;
    int lane = -1;                     // the gate's lane that carries the batch in flight and still counts it, -1: none
    bool on_lane = false;              // the batch in flight runs on a lane (which may carry other contexts' batches)
    ocvar::Event ev[ocvar::EV_COUNT];
    ocvar::Event ordered;              // orders a lane behind the caller's work on `stream` (created on first use)
    // A batch on a lane: collect waits for events, not for a stream.  `copied` lies behind the results copies made with stream
    // NULL or on the context's own stream -- collect used to cover both, they were the batch's stream then.
    ocvar::Event copied;               // (created on first use)
    bool copy_pending = false;
    ocvar::Event h2d_done[2];          // host transport: a staging slot's upload (created on first use)
    // the workspaces of the frame operations (frame_ops.hip): render_records reads the overlay table and images too
    ocvar::WorkspaceFence ovl_fence, anno_fence, levels_fence, flow_fence;
    std::vector<void*> allocs;         // the workspace's arrays of fixed size (dev_alloc), freed with the context
    ocvar::DeviceBuffer<long long> sq_codes;   // ws.sq_codes / ws.sq_match, which mirror them: they grow with the library
    ocvar::DeviceBuffer<int> sq_match;
    ocvar::DeviceBuffer<uint8_t> d_frames;     // staging for the host-buffer entry points
    ocvar::PinnedBuffer<uint8_t> h_stage[2];   // page-locked staging of the host entry points (double buffer)
    ocvar::PinnedBuffer<uint8_t> h_grey[2];    // page-locked staging of the in-place grey on its way back (double buffer)
    ocvar::PinnedBuffer<ocvar::MarkerRec> h_markers;
    ocvar::PinnedBuffer<ocvar::MarkerRec> h_prev;   // the caller's previous markers on their way to the device
    ocvar::PinnedBuffer<int> h_prev_counts;
    ocvar::PinnedBuffer<int> h_counts;
    ocvar::PinnedBuffer<int> h_counters;
    bool pending = false;
    bool crops_ran = false;            // the last batch ran the crop pass (ocvar_hip_debug_crop_*: its ROIs and planes are in the workspace)
    bool have_templates = false, have_camera = false;
    ocvar::CameraRec h_camera{};   // the camera as last set, for the entry points that pass it by value (ocvar_hip_undistort)
    ocvar::Library lib;       // the templates' table as uploaded (ocvar_hip_debug_candidates expands a square with it)
    int capacity_flags = 0;   // flag word of the last batch that failed with OCVAR_E_CAPACITY
    // planar board (ocvar_hip_set_board): the device table is allocated by the first board set
    int board_n = 0;                               // entries of the next batch's board, 0: off
    ocvar::BoardEntry* d_board = nullptr;          // [OCVAR_MAX_BOARD_MARKERS]
    int* d_board_map = nullptr;                    // [MAXT] templateId -> board index, -1
    ocvar::BoardPose* d_board_poses = nullptr;     // [max_batch]
    ocvar::PinnedBuffer<ocvar::BoardPose> h_board_poses;   // [max_batch]
    bool batch_board = false;                      // the enqueued batch runs the board kernel
    std::vector<ocvar::BoardPose> board_out;       // the poses of the last collected batch (ocvar_hip_board_poses)
    bool board_out_valid = false;
    int board_out_off = 0;                         // where collect puts a batch's poses in board_out (detect_host's sub-batches)
    // overlays (ocvar_hip_set_overlay): table and drawing workspace are allocated by the first overlay set
    ocvar::OverlayTable* h_overlays = nullptr;     // the table as uploaded (device pointers inside: ~OcvarHip frees them)
    ocvar::OverlayTable* d_overlays = nullptr;
    ocvar::OverlayDraw* d_ovl_draws = nullptr;     // [max_batch][maxm]
    ocvar::OverlayBox* d_ovl_boxes = nullptr;      // [max_batch][maxm]
    int n_overlays = 0;
    // flow tracking (ocvar_hip_flow_records): the pyramids' workspace is allocated by the first call
    ocvar::DeviceBuffer<uint8_t> flow_ws;          // [2][min(max_batch, 32)] pyramids of a max_w x max_h frame (flow_core.h: flow_geom)
    // annotation (ocvar_hip_annotate / ocvar_hip_annotate_records): the primitive records' workspace is allocated by the first call
    ocvar::DeviceBuffer<ocvar::AnnoRec> anno_recs; // [max_batch][maxm]
    ocvar::DeviceBuffer<ocvar::AnnoBox> anno_boxes;   // [max_batch][maxm]
    // levels (ocvar_hip_levels): the tile histograms and LUTs' workspace is allocated, and cleared, by the first call
    ocvar::DeviceBuffer<uint8_t> levels_ws;        // levels_core.h: LEVELS_WS_BYTES
    std::string err;

    ~OcvarHip();   // (api.hip: the fixed arrays and the overlay images; the holders release the rest)
};

#define HIP_TRY(ctx, call)                                                                              \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
            return OCVAR_E_HIP;                                                                         \
        }                                                                                               \
    } while (0)

// OCVAR_TRACE_LAUNCHES=1: wait after every launch and name it on stderr (locating a faulting or hanging kernel)
#define TRACE_LAUNCH(name, st)                                                             \
    do {                                                                                 \
        if (ocvar::trace_launches()) {                                                   \
            std::fprintf(stderr, "ocvar: %s ...", name);                                 \
            std::fflush(stderr);                                                         \
            hipError_t e_ = hipStreamSynchronize(st);                                    \
            std::fprintf(stderr, " %s\n", e_ == hipSuccess ? "ok" : hipGetErrorString(e_)); \
        }                                                                                \
    } while (0)

namespace ocvar {

// One batch as its caller asks for it: frames in device memory in `format` (OCVAR_FMT_*), the previous step's markers (host
// memory, or device memory with prev_on_device; null: none), and how far the chain runs (stages 3: detection, 2: up to the
// ordered squares, 0: the frame binarise kernel only).
struct BatchRequest {
    uint8_t* frames;
    int width, height, row_stride;
    size_t frame_stride;
    int n_frames, grey_in_place;
    const OcvarMarker* prev;
    const int* prev_counts;
    bool prev_on_device;
    int format, stages;
};

// api.hip
bool trace_launches();
int refuse_if_pending(OcvarHip* c);   // OCVAR_E_ARG and the error text while a batch awaits its collect
int frame_span_check(OcvarHip* c, int width, int height, int row_stride, int format);
// the batch on stream s; `after`: a stream whose work in flight the batch follows (null: none)
int enqueue_impl(OcvarHip* c, const BatchRequest& r, hipStream_t s, hipStream_t after);
hipError_t batch_wait(OcvarHip* c);
int wait_impl(OcvarHip* c);
// Work that follows the batch in flight lies between follow_begin (the stream it goes to, ordered behind the batch) and follow_end
int follow_begin(OcvarHip* c, void* stream, hipStream_t* s);
int follow_end(OcvarHip* c, hipStream_t s);
bool batch_frames_ok(OcvarHip* c, const char* who, int width, int height);   // false and the text: no batch, or frames of another size
// n elements (and a margin) of device memory that live as long as the context
template <typename T>
int dev_alloc(OcvarHip* c, T** p, size_t n) {
    void* q = nullptr;
    HIP_TRY(c, hipMalloc(&q, n * sizeof(T) + 256));
    c->allocs.push_back(q);
    *p = static_cast<T*>(q);
    return OCVAR_OK;
}
// gate.hip
void gate_detach(OcvarHip* c);
void lane_release(OcvarHip* c);
int gate_place(OcvarGate* g);
hipError_t gate_enter(OcvarGate* g, hipStream_t s);
hipError_t gate_leave(OcvarGate* g, hipStream_t s);
// debug.hip: the first min(*n_quads, lim) ordered squares of a frame of the last batch as integer quads
int quads_to_host(OcvarHip* c, int frame, int lim, int* quads, int* n_quads);

}  // namespace ocvar
