// api.hip -- the thin C ABI of include/ocvar_hip.h: context, device workspace, templates, camera and tuning, launch sequence,
// result copy-out, board setup, timing and counters.  (context.h: the context itself; plan_core.h: sizes and grids; frame_ops.hip:
// the opt-in operations on frames and records; gate.hip, host_transport.hip, debug.hip: the gate and its lanes, frames in host
// memory, the debug entry points.)
//
// One batch = 12 kernel launches on one HIP stream, no host round trip in between (work counts stay in
// device memory and the second-pass kernels are launched with fixed grids that read them):
//   binarise(frames) -> follower tiers 1,2,3 (frames) -> order+crops -> binarise(crops) -> follower tiers 1, 2 (two phases:
//   follow.hip), 3 (crops) -> decode -> finalise
// There is deliberately no CPU path here: if the device or the code object is missing, create() fails.
#include "context.h"
#include "frames_core.h"
#include "plan_core.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>

using namespace ocvar;

static_assert(sizeof(TemplateRec) == sizeof(OcvarTemplate) && sizeof(TemplateRec) == 48, "CvarTemplate layout");
static_assert(MAX_SIZE_CLASSES == OCVAR_MAX_TEMPLATE_SIZES, "size classes");
static_assert(sizeof(CameraRec) == sizeof(OcvarCamera) && sizeof(CameraRec) == 248, "CvarCamera layout");
static_assert(sizeof(MarkerRec) == sizeof(OcvarMarker) && sizeof(MarkerRec) == 184, "CvarMarker layout");
static_assert(sizeof(BoardEntry) == sizeof(OcvarBoardMarker) && sizeof(BoardEntry) == 72, "OcvarBoardMarker layout");
static_assert(sizeof(BoardPose) == sizeof(OcvarBoardPose) && sizeof(BoardPose) == 192, "OcvarBoardPose layout");

static int create_impl(OcvarHip** out, int device, int max_width, int max_height, int max_batch, int max_quads, int max_markers,
                       bool dense) {
    // (corner points travel packed as x | y << 16 through the follower tiers: coordinates stay below 2^15)
    if (!out || max_width < 16 || max_height < 16 || max_width > 32767 || max_height > 32767 || max_batch < 1 || max_quads < 1 ||
        max_markers < 1)
        return OCVAR_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return OCVAR_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return OCVAR_E_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "ocvar_hip: device %d is %s; this library carries gfx950 code only\n", device, prop.gcnArchName);
        return OCVAR_E_NO_DEVICE;
    }
    OcvarHip* c = new (std::nothrow) OcvarHip();
    if (!c) return OCVAR_E_HIP;
    *out = c;  // returned even on failure below so the caller can read the error text, then destroy
    c->device = device;
    HIP_TRY(c, hipSetDevice(device));
    HIP_TRY(c, c->stream.ensure(hipStreamNonBlocking));
    for (auto& e : c->ev) HIP_TRY(c, e.ensure(hipEventDefault));
    Workspace& w = c->ws;
    plan_workspace(&w, max_width, max_height, max_batch, max_quads, max_markers, dense);
    c->result_limit = max_markers;
    const size_t B = (size_t)max_batch, M = (size_t)max_markers;
    int rc;
    if ((rc = dev_alloc(c, &w.gray, B * (size_t)gray_plane_bytes(max_width, max_height)))) return rc;   // (panels: hd.h::gray_col)
    if ((rc = dev_alloc(c, &w.nbr_frame, B * (size_t)nbr_plane_bytes(((max_width & ~1) + 15) & ~15, max_height & ~1)))) return rc;
    if ((rc = dev_alloc(c, &w.nbr_crop, (size_t)w.cap_crop_pixels))) return rc;
    if ((rc = dev_alloc(c, &w.cands_frame, (size_t)w.cap_frame_cands))) return rc;
    if ((rc = dev_alloc(c, &w.cands_crop, (size_t)w.cap_crop_cands))) return rc;
    if ((rc = dev_alloc(c, &w.pool, (size_t)w.cap_pool_ints))) return rc;
    if ((rc = dev_alloc(c, &w.slab, (size_t)w.max_mid_blocks * 256 * SLAB_STRIDE))) return rc;
    if ((rc = dev_alloc(c, &w.slab3, (size_t)w.max_long_blocks * 4 * SLAB3_STRIDE))) return rc;
    if ((rc = dev_alloc(c, &w.mid_frame, (size_t)w.cap_long))) return rc;
    if ((rc = dev_alloc(c, &w.mid_crop, (size_t)w.cap_long))) return rc;
    if ((rc = dev_alloc(c, &w.mid_first_crop, (size_t)w.cap_long))) return rc;
    if ((rc = dev_alloc(c, &w.crop_early, (size_t)w.cap_long))) return rc;
    if ((rc = dev_alloc(c, &w.crop_rest, (size_t)w.cap_long))) return rc;
    if ((rc = dev_alloc(c, &w.crop_live, (size_t)w.cap_long))) return rc;
    if ((rc = dev_alloc(c, &w.long_frame, (size_t)w.cap_long))) return rc;
    if ((rc = dev_alloc(c, &w.long_crop, (size_t)w.cap_long))) return rc;
    if ((rc = dev_alloc(c, &w.quads_frame, B * max_quads))) return rc;
    if ((rc = dev_alloc(c, &w.n_quads_frame, B))) return rc;
    if ((rc = dev_alloc(c, &w.squares, B * max_quads * 8))) return rc;
    if ((rc = dev_alloc(c, &w.n_squares, B))) return rc;
    if ((rc = dev_alloc(c, &w.crop_of, B * max_quads))) return rc;
    if ((rc = dev_alloc(c, &w.rois_crop, (size_t)w.cap_crop_rois))) return rc;
    if ((rc = dev_alloc(c, &w.tiles_crop, (size_t)w.cap_crop_tiles))) return rc;
    if ((rc = dev_alloc(c, &w.quads_crop, (size_t)w.cap_crop_quads))) return rc;
    if ((rc = dev_alloc(c, &w.best_crop, (size_t)w.cap_crop_rois))) return rc;
    if ((rc = dev_alloc(c, &w.crop_min_rest, (size_t)w.cap_crop_rois))) return rc;
    if ((rc = dev_alloc(c, &w.ring_frame, B))) return rc;
    if ((rc = dev_alloc(c, &w.ring_crop, (size_t)w.cap_crop_rois))) return rc;
    if ((rc = dev_alloc(c, &w.sq_recs, B * max_quads))) return rc;   // (sq_codes, sq_match: ocvar_hip_set_templates)
    if ((rc = dev_alloc(c, &w.prev, B * M))) return rc;
    if ((rc = dev_alloc(c, &w.n_prev, B))) return rc;
    if ((rc = dev_alloc(c, &w.reserve, B * M))) return rc;
    if ((rc = dev_alloc(c, &w.n_reserve, B))) return rc;
    if ((rc = dev_alloc(c, &w.markers, B * M))) return rc;
    if ((rc = dev_alloc(c, &w.pose_jobs, B * M))) return rc;
    if (dense) {   // the scalable tail (follow.hip: order_sort .. crops_kernel; decode.hip: finalise_kernel<true>)
        const int nc = w.track_gw * w.track_gh;
        if ((rc = dev_alloc(c, &w.sorted_starts, B * max_quads))) return rc;
        if ((rc = dev_alloc(c, &w.sq_tmp, B * max_quads * 8))) return rc;
        if ((rc = dev_alloc(c, &w.trk_cells, B * (nc + 1)))) return rc;
        if ((rc = dev_alloc(c, &w.trk_fill, B * nc))) return rc;
        if ((rc = dev_alloc(c, &w.trk_items, B * 4 * max_quads))) return rc;
        if ((rc = dev_alloc(c, &w.trk_next, B * (max_quads + 1)))) return rc;
        if ((rc = dev_alloc(c, &w.surv, B * max_quads))) return rc;
        if ((rc = dev_alloc(c, &w.src, B * M))) return rc;
    }
    if ((rc = dev_alloc(c, &w.n_markers, B))) return rc;
    if ((rc = dev_alloc(c, &w.templates, (size_t)MAXT))) return rc;
    if ((rc = dev_alloc(c, &w.sizes, (size_t)MAX_SIZE_CLASSES))) return rc;
    if ((rc = dev_alloc(c, &w.lut, (size_t)4 * MAXT))) return rc;
    if ((rc = dev_alloc(c, &w.group_off, (size_t)MAXT + 1))) return rc;
    if ((rc = dev_alloc(c, &w.group_members, (size_t)MAXT))) return rc;
    if ((rc = dev_alloc(c, &w.camera, (size_t)1))) return rc;
    if ((rc = dev_alloc(c, &w.counters, (size_t)CNT_COUNT))) return rc;

    w.crop_pixels = reinterpret_cast<unsigned long long*>(w.counters + CNT_CROP_PIXELS);
    HIP_TRY(c, hipMemset(w.n_prev, 0, B * sizeof(int)));
    HIP_TRY(c, hipMemset(w.counters, 0, CNT_COUNT * sizeof(int)));
    HIP_TRY(c, c->h_markers.reserve(B * M * sizeof(MarkerRec)));
    HIP_TRY(c, c->h_counts.reserve(B * sizeof(int)));
    HIP_TRY(c, c->h_prev.reserve(B * M * sizeof(MarkerRec)));
    HIP_TRY(c, c->h_prev_counts.reserve(B * sizeof(int)));
    HIP_TRY(c, c->h_counters.reserve(CNT_COUNT * sizeof(int)));
    return OCVAR_OK;
}

extern "C" int ocvar_hip_create(OcvarHip** out, int device, int max_width, int max_height, int max_batch) {
    return ocvar_hip_create_ex(out, device, max_width, max_height, max_batch, OCVAR_MAX_QUADS);
}

extern "C" int ocvar_hip_create_ex(OcvarHip** out, int device, int max_width, int max_height, int max_batch, int max_quads) {
    if (max_quads < 1 || max_quads > OCVAR_MAX_QUADS_EX) return OCVAR_E_ARG;
    return create_impl(out, device, max_width, max_height, max_batch, max_quads, OCVAR_MAX_MARKERS, false);
}

extern "C" int ocvar_hip_create_dense(OcvarHip** out, int device, int max_width, int max_height, int max_batch, int max_quads,
                                      int max_markers) {
    // (the arguments are checked before any device call)
    if (max_quads < 1 || max_quads > OCVAR_MAX_QUADS_DENSE || max_markers < 1 || max_markers > OCVAR_MAX_MARKERS_DENSE) return OCVAR_E_ARG;
    return create_impl(out, device, max_width, max_height, max_batch, max_quads, max_markers, true);
}

extern "C" int ocvar_hip_max_markers(const OcvarHip* c) { return c ? c->ws.maxm : OCVAR_E_ARG; }

// What no holder owns: the workspace's fixed arrays, and the overlay images inside the table (a plain record the kernels read:
// its pointers are raw) with the table.
OcvarHip::~OcvarHip() {
    for (void* p : allocs) (void)hipFree(p);
    if (!h_overlays) return;
    for (auto& t : h_overlays->tex)
        if (t.px) (void)hipFree(const_cast<uint32_t*>(t.px));
    delete h_overlays;
}

extern "C" void ocvar_hip_destroy(OcvarHip* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    gate_detach(c);   // (waits for a batch on a lane of the gate)
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    // (a frame operation in flight uses its workspace; a render_records reads the overlay images too)
    for (WorkspaceFence* f : {&c->ovl_fence, &c->anno_fence, &c->levels_fence, &c->flow_fence}) (void)f->drain();
    delete c;
}

// Waits for the batch in flight as collect does: on a lane for its own last event and for the results copies made on the lane
// or on the context's own stream (the lane may carry the next context's batch by now); elsewhere for the batch's stream.
hipError_t ocvar::batch_wait(OcvarHip* c) {
    if (!c->on_lane) return hipStreamSynchronize(c->last_stream);
    return hipEventSynchronize(c->copy_pending ? c->copied : c->ev[EV_LAST]);   // (`copied` is behind ev[EV_LAST] on the lane)
}

extern "C" void* ocvar_hip_stream(const OcvarHip* c) { return c ? (void*)c->stream.s : nullptr; }

extern "C" const char* ocvar_hip_last_error(const OcvarHip* c) { return c ? c->err.c_str() : "null context"; }
extern "C" int ocvar_hip_capacity_flags(const OcvarHip* c) { return c ? c->capacity_flags : 0; }

extern "C" int ocvar_hip_set_templates(OcvarHip* c, const OcvarTemplate* t, int n) {
    if (!c) return OCVAR_E_ARG;
    if (!t || n < 1 || n > MAXT) {
        c->err = "ocvar_hip_set_templates: need 1.." + std::to_string(MAXT) + " templates";
        return OCVAR_E_ARG;
    }
    for (int i = 0; i < n; i++)
        if (t[i].width < 1 || t[i].height < 1 || t[i].width * t[i].height > 64) {
            c->err = "ocvar_hip_set_templates: template " + std::to_string(i) + " is not 1..64 code cells";
            return OCVAR_E_ARG;
        }
    Library lib;
    if (!build_library(reinterpret_cast<const TemplateRec*>(t), n, &lib)) {
        c->err = "ocvar_hip_set_templates: more than " + std::to_string(MAX_SIZE_CLASSES) + " distinct template sizes";
        return OCVAR_E_ARG;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->pending) HIP_TRY(c, batch_wait(c));   // (the batch in flight reads the tables)
    Workspace& w = c->ws;
    const size_t squares = (size_t)w.max_batch * w.maxq;
    c->have_templates = false;   // (until the tables below are all in place)
    // (per-square arrays that grow with the library; the workspace's pointers mirror their owners, whatever the outcome)
    hipError_t grown = c->sq_codes.reserve(squares * lib.sizes.size() * sizeof(long long));
    if (grown == hipSuccess) grown = c->sq_match.reserve(squares * lib.max_match * sizeof(int));
    w.sq_codes = c->sq_codes;
    w.sq_match = c->sq_match;
    HIP_TRY(c, grown);
    HIP_TRY(c, hipMemcpy(w.templates, t, n * sizeof(OcvarTemplate), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(w.sizes, lib.sizes.data(), lib.sizes.size() * sizeof(SizeClass), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(w.lut, lib.lut.data(), lib.lut.size() * sizeof(LutEntry), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(w.group_off, lib.group_off.data(), lib.group_off.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(w.group_members, lib.members.data(), lib.members.size() * sizeof(int), hipMemcpyHostToDevice));
    w.n_templates = n;
    w.n_sizes = (int)lib.sizes.size();
    w.n_groups = lib.n_groups();
    w.max_match = lib.max_match;
    c->lib = std::move(lib);
    c->have_templates = true;
    return OCVAR_OK;
}

extern "C" int ocvar_hip_set_camera(OcvarHip* c, const OcvarCamera* cam) {
    if (!c || !cam) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(c->ws.camera, cam, sizeof(OcvarCamera), hipMemcpyHostToDevice));
    std::memcpy(&c->h_camera, cam, sizeof(OcvarCamera));
    c->have_camera = true;
    return OCVAR_OK;
}

// Where a result-invariant launch parameter comes from: the context's own setting (ocvar_hip_set_tuning), else none -- the
// default holds (plan_core.h says what a value means).  Profiling builds (-DOCVAR_PROF) also listen to the environment variable
// of the same purpose; the product library reads no tuning from the environment, so a benchmark number cannot depend on the
// caller's shell.
constexpr int HP_MASK_DEFAULT = 0;

static PlanKnob tuned(const OcvarHip* c, int knob, const char* env_name) {
    if (knob > 0 && knob < TUNE_KNOBS && c->tune[knob] > 0) return {true, knob == OCVAR_TUNE_HP_MASK ? c->tune[knob] - 1 : c->tune[knob]};
#ifdef OCVAR_PROF
    if (const char* e = std::getenv(env_name)) return {true, std::atoll(e)};
#else
    (void)env_name;
#endif
    return {false, 0};
}

extern "C" int ocvar_hip_set_tuning(OcvarHip* c, int knob, int value) {
    if (!c || knob < 1 || knob >= TUNE_KNOBS || value < 0 || c->pending) return OCVAR_E_ARG;
    c->tune[knob] = knob == OCVAR_TUNE_HP_MASK ? value + 1 : value;   // (0 is a meaningful mask: stored off by one, 0 = default)
    return OCVAR_OK;
}

extern "C" const char* ocvar_hip_build_info(void) {
    return "libocvar_hip gfx950"
#ifdef OCVAR_NBR_TILED
           " OCVAR_NBR_TILED"
#endif
#ifdef OCVAR_PROF
           " OCVAR_PROF(env tuning + knock-out switches + cycle counters: NOT a product build)"
#else
           " product(no environment tuning, no knock-out switches; OCVAR_TRACE_LAUNCHES only)"
#endif
        ;
}

bool ocvar::trace_launches() {
    static const bool on = std::getenv("OCVAR_TRACE_LAUNCHES") != nullptr;
    return on;
}

int ocvar::refuse_if_pending(OcvarHip* c) {
    if (!c->pending) return OCVAR_OK;
    c->err = "the previous batch of this context has not been collected";
    return OCVAR_E_ARG;
}

// A frame whose rows reach further from its first byte than the frame binarise kernel addresses (hd.h::frame_src_addressable)
// is refused: its lower rows would be read somewhere else, or as zeros, and the call would return a plausible, different result.
int ocvar::frame_span_check(OcvarHip* c, int width, int height, int row_stride, int format) {
    const int bpp = format_bpp(format);
    if (frame_src_addressable(width, height, row_stride, bpp)) return OCVAR_OK;
    c->err = "the rows of a frame span more than the frame kernel addresses: ((height & ~1) - 1) * row_stride + bytes per pixel * "
             "(width & ~1) must not exceed 2147483647 (got " +
             std::to_string(((long long)(height & ~1) - 1) * row_stride + (long long)bpp * (width & ~1)) + ")";
    return OCVAR_E_ARG;
}

// The first per_frame marker records of every frame of the batch to dst, where a frame's records lie dst_stride records after
// the frame's before: one block when that is all of them, else a strided copy.
static hipError_t copy_markers(const Workspace& w, void* dst, int dst_stride, int per_frame, hipMemcpyKind kind, hipStream_t s) {
    constexpr size_t R = sizeof(MarkerRec);
    if (per_frame >= w.maxm) return hipMemcpyAsync(dst, w.markers, (size_t)w.n_frames * w.maxm * R, kind, s);
    return hipMemcpy2DAsync(dst, dst_stride * R, w.markers, w.maxm * R, per_frame * R, (size_t)w.n_frames, kind, s);
}

int ocvar::enqueue_impl(OcvarHip* c, const BatchRequest& r, hipStream_t s, hipStream_t after) {
    Workspace& w = c->ws;
    const int n_frames = r.n_frames;
    int stages = r.stages;
    if (!r.frames || r.width < 16 || r.height < 16 || r.width > w.max_w || r.height > w.max_h || n_frames < 1 || n_frames > w.max_batch ||
        (size_t)r.width * r.height > (size_t)w.max_w * w.max_h || format_bpp(r.format) == 0 ||
        (long long)r.row_stride < (long long)format_bpp(r.format) * r.width)
        return OCVAR_E_ARG;
    if (int rc = frame_span_check(c, r.width, r.height, r.row_stride, r.format)) return rc;
    if (int rc = refuse_if_pending(c)) return rc;
    if (stages > 2 && (!c->have_templates || !c->have_camera)) {
        c->err = "templates and camera must be set before detection";
        return OCVAR_E_ARG;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    c->batch_board = false;
    c->crops_ran = false;   // (from here on the workspace belongs to this batch)
    plan_batch(&w, r.width, r.height, n_frames, c->gate != nullptr,
               PlanOverrides{tuned(c, OCVAR_TUNE_CROP_PHASES, "OCVAR_CROP_PHASES"), tuned(c, OCVAR_TUNE_MID_STEPS, "OCVAR_MID_STEPS"),
                             tuned(c, OCVAR_TUNE_MID_BLOCKS, "OCVAR_MID_BLOCKS"), tuned(c, OCVAR_TUNE_LONG_BLOCKS, "OCVAR_LONG_BLOCKS"),
                             tuned(c, OCVAR_TUNE_SHORT_BLOCKS, "OCVAR_SHORT_BLOCKS"), tuned(c, OCVAR_TUNE_MIN_UNITS, "OCVAR_MIN_UNITS")});
    if (after && after != s && hipStreamQuery(after) != hipSuccess) {
        // The batch runs on a lane, and the caller has work in flight on the context's stream (frames being written, a wait for
        // an event of theirs, the last batch's results on their way out): the batch follows it.  An idle stream asks for
        // nothing, and nothing is put into its hardware queue -- a record there would queue up behind the lane that shares it.
        (void)hipGetLastError();   // (not ready: no error)
        HIP_TRY(c, c->ordered.ensure(hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->ordered, after));
        HIP_TRY(c, hipStreamWaitEvent(s, c->ordered, 0));
    }
    HIP_TRY(c, hipMemsetAsync(w.counters, 0, CNT_COUNT * sizeof(int), s));
    HIP_TRY(c, hipMemsetAsync(w.n_quads_frame, 0, n_frames * sizeof(int), s));
    if (r.prev && r.prev_counts && r.prev_on_device) {
        // the previous step's markers never left the device (ocvar_hip_enqueue_tracked: streams of a tracker)
        HIP_TRY(c, hipMemcpyAsync(w.prev, r.prev, (size_t)n_frames * w.maxm * sizeof(MarkerRec), hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(w.n_prev, r.prev_counts, n_frames * sizeof(int), hipMemcpyDeviceToDevice, s));
    } else if (r.prev && r.prev_counts) {
        // through the context's page-locked buffers: the device never touches the caller's (pageable, possibly tiny) arrays.
        // (A batch is collected before the next one is enqueued on a context, so the buffers are free again by then.)
        std::memcpy(c->h_prev, r.prev, (size_t)n_frames * w.maxm * sizeof(MarkerRec));
        std::memcpy(c->h_prev_counts, r.prev_counts, n_frames * sizeof(int));
        HIP_TRY(c, hipMemcpyAsync(w.prev, c->h_prev, (size_t)n_frames * w.maxm * sizeof(MarkerRec), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(w.n_prev, c->h_prev_counts, n_frames * sizeof(int), hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(c, hipMemsetAsync(w.n_prev, 0, n_frames * sizeof(int), s));
    }
    // Which kernels run on the context's high-priority stream (OCVAR_TUNE_HP_MASK, one bit per launch after the first
    // binarise kernel: 1 tier 1 (frames), 2 tier 2, 4 tier 3, 8 order/crops, 16 tier 1 (crops), 32 tier 2, 64 tier 3, 128 decode,
    // 256 dedupe+pose).  With several contexts in flight a binarise kernel of another context has tens of thousands of
    // 80-register workgroups queued, and every slot a finished one frees is refilled from that queue at once: a kernel with a
    // larger footprint -- decode and dedupe+pose: 256 / 64 threads at 128 registers -- finds room only by accident and takes 6 ms
    // in-region for 0.3 ms of work, at the end of its context's chain.  On a high-priority queue its workgroups are placed
    // first.  (All followers on the high-priority stream -- round 2's OCVAR_SPLIT_STREAMS -- halved their in-region durations and
    // lengthened binarise's by as much; the mask chooses kernel by kernel.)  The events that time the stages also order the
    // streams.
    const int hp_mask = (int)knob_or(tuned(c, OCVAR_TUNE_HP_MASK, "OCVAR_HP_MASK"), HP_MASK_DEFAULT) & 0x1ff;
    if (hp_mask && !c->hp_stream) {
        int lo = 0, hi = 0;
        HIP_TRY(c, hipDeviceGetStreamPriorityRange(&lo, &hi));   // hi: numerically lowest = greatest priority
        HIP_TRY(c, hipStreamCreateWithPriority(&c->hp_stream.s, hipStreamNonBlocking, hi));
    }
    hipStream_t cur = s;   // the stream the chain is on
    auto stage = [&](int k, int bit) -> hipError_t {   // timing event k at the end of the previous stage; the next one runs where its bit says
        hipStream_t to = (bit >= 0 && ((hp_mask >> bit) & 1)) ? c->hp_stream.s : s;
        hipError_t e = hipEventRecord(c->ev[k], cur);
        if (e == hipSuccess && to != cur) e = hipStreamWaitEvent(to, c->ev[k], 0);
        cur = to;
        return e;
    };
    const int gate_mode = (int)knob_or(tuned(c, OCVAR_TUNE_GATE_MODE, "OCVAR_GATE_MODE"), 0);   // which binarise kernels the gate covers: 0 both, 1 the frames kernel only, 2 the crops kernel only
    if (gate_mode != 2) HIP_TRY(c, gate_enter(c->gate, s));   // (before the first timing event: a wait at the gate is not binarise time)
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    launch_binarise_frames(w, r.frames, r.row_stride, r.frame_stride, r.grey_in_place, r.format, s);
    if (gate_mode != 2) HIP_TRY(c, gate_leave(c->gate, s));
    TRACE_LAUNCH("binarise_frames", s);
    // Timing experiments (results are then incomplete or wrong): compiled into profiling builds only (-DOCVAR_PROF, `make prof`)
    //   OCVAR_ONLY_BINARISE=1        stop after the first kernel (tools/binarise_only.py)
    //   OCVAR_SKIP_CROP_KERNELS=bits knock out kernels of the crop pass: 1 binarise_crops, 2 tier 1, 4 tier 2, 8 tier 3
#ifdef OCVAR_PROF
    static const bool only_binarise = std::getenv("OCVAR_ONLY_BINARISE") != nullptr;
    static const int skip_crop = std::getenv("OCVAR_SKIP_CROP_KERNELS") ? std::atoi(std::getenv("OCVAR_SKIP_CROP_KERNELS")) : 0;
    if (only_binarise || skip_crop) {
        static bool warned = false;
        if (!warned) std::fprintf(stderr, "ocvar_hip: OCVAR_ONLY_BINARISE / OCVAR_SKIP_CROP_KERNELS set -- timing experiment, detection results are NOT valid\n");
        warned = true;
    }
#else
    constexpr bool only_binarise = false;
    constexpr int skip_crop = 0;
#endif
    if (only_binarise) stages = 0;
    if (stages > 0) {
        HIP_TRY(c, stage(1, 0));
        // (one frame per call: two more launches cost more than the walks they save -- the wave tier crosses a clean frame border 64
        // pixels at a time --: 2.37 -> 2.47 ms per 1080p call measured; batches: tier 3 on frames 0.32 -> 0.15 ms, tier 2 on crops -8 %)
        if (n_frames > 8) launch_ring_quads_frames(w, cur);
        else HIP_TRY(c, hipMemsetAsync(w.ring_frame, 0, n_frames * sizeof(int), cur));
        launch_follow_frames(w, cur);
        TRACE_LAUNCH("follow tier 1 (frames)", cur);
        HIP_TRY(c, stage(2, 1));
        launch_follow_mid_frames(w, cur);
        TRACE_LAUNCH("follow tier 2 (frames)", cur);
        HIP_TRY(c, stage(3, 2));
        launch_follow_long_frames(w, cur);
        TRACE_LAUNCH("follow tier 3 (frames)", cur);
        HIP_TRY(c, stage(4, 3));
        launch_order_and_crops(w, cur);
        TRACE_LAUNCH("order_and_crops", cur);
    } else {
        for (int k = 1; k < 5; k++) HIP_TRY(c, hipEventRecord(c->ev[k], s));
    }
    if (stages > 2) {
        // (the gate wait is enqueued on s before s is made to wait for the order kernel: a wait here is booked under the
        // order_crops interval)
        if (gate_mode != 1) HIP_TRY(c, gate_enter(c->gate, s));
        HIP_TRY(c, stage(5, -1));
        if (!(skip_crop & 1)) launch_binarise_crops(w, s);
        if (gate_mode != 1) HIP_TRY(c, gate_leave(c->gate, s));
        TRACE_LAUNCH("binarise_crops", s);
        HIP_TRY(c, stage(6, 4));
        if (!(skip_crop & 2) && n_frames > 8) launch_ring_quads_crops(w, cur);   // (else: order_and_crops_kernel cleared the crops' flags)
        if (!(skip_crop & 2)) launch_follow_crops(w, cur);
        TRACE_LAUNCH("follow tier 1 (crops)", cur);
        HIP_TRY(c, stage(7, 5));
        if (!(skip_crop & 4)) launch_follow_mid_crops(w, cur);
        TRACE_LAUNCH("follow tier 2 (crops)", cur);
        HIP_TRY(c, stage(8, 6));
        if (!(skip_crop & 8)) launch_follow_long_crops(w, cur);
        TRACE_LAUNCH("follow tier 3 (crops)", cur);
        HIP_TRY(c, stage(9, 7));
        launch_decode(w, cur);
        TRACE_LAUNCH("decode", cur);
        HIP_TRY(c, stage(10, 8));
        launch_finalise(w, c->refine, cur);
        TRACE_LAUNCH("finalise", cur);
        HIP_TRY(c, stage(11, -1));
        if (c->board_n > 0) {   // (no board: no launch, no copy)
            launch_board_poses(w, BoardArgs{c->board_n, c->d_board, c->d_board_map, c->d_board_poses}, s);
            TRACE_LAUNCH("board", s);
            HIP_TRY(c, hipMemcpyAsync(c->h_board_poses, c->d_board_poses, n_frames * sizeof(BoardPose), hipMemcpyDeviceToHost, s));
            c->batch_board = true;
        }
        HIP_TRY(c, hipMemcpyAsync(c->h_counts, w.n_markers, n_frames * sizeof(int), hipMemcpyDeviceToHost, s));
        // (the first result_limit records of every frame, at their usual places in the host block)
        HIP_TRY(c, copy_markers(w, c->h_markers, w.maxm, c->result_limit, hipMemcpyDeviceToHost, s));
    } else {
        HIP_TRY(c, stage(5, -1));
        for (int k = 6; k < EV_LAST; k++) HIP_TRY(c, hipEventRecord(c->ev[k], s));
    }
    HIP_TRY(c, hipMemcpyAsync(c->h_counters, w.counters, CNT_COUNT * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(c->ev[EV_LAST], s));
    HIP_TRY(c, hipGetLastError());
    c->last_stream = s;
    c->copy_pending = false;
    c->pending = true;
    c->crops_ran = stages > 2;
    return OCVAR_OK;
}

// ocvar_hip_enqueue / _tracked: the stream the caller names; else, for a context of a gate, the gate's lane with the least
// outstanding work; else the context's own stream.
static int enqueue_placed(OcvarHip* c, const BatchRequest& r, void* stream) {
    OcvarGate* g = c->gate;
    if (stream || !g || c->pending)   // (pending: enqueue_impl refuses)
        return enqueue_impl(c, r, stream ? (hipStream_t)stream : c->stream.s, nullptr);
    HIP_TRY(c, hipSetDevice(c->device));
    const int lane = gate_place(g);   // (booked: the context's `lane` must name it before anybody looks)
    c->lane = lane;
    const int rc = enqueue_impl(c, r, g->lanes[lane], c->stream);
    if (rc == OCVAR_OK) c->on_lane = true;
    else lane_release(c);
    return rc;
}

int ocvar::wait_impl(OcvarHip* c) {
    if (!c->pending) {
        c->err = "nothing enqueued";
        return OCVAR_E_ARG;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, batch_wait(c));
    c->pending = false;
    c->on_lane = false;
    lane_release(c);
    const int e = c->h_counters[CNT_ERR];
    c->capacity_flags = e;
    if (e) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "device work list overflow / trace overrun, flags 0x%x (1 starts, 2 point pool, 4 quads, 8 overrun, 16 crops, 32 tiles, 64 ticket runaway, 128 markers)", e);
        c->err = buf;
        return OCVAR_E_CAPACITY;
    }
    return OCVAR_OK;
}

extern "C" int ocvar_hip_enqueue(OcvarHip* c, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride,
                                 int n_frames, int grey_in_place, const OcvarMarker* prev, const int* prev_counts, void* stream) {
    if (!c) return OCVAR_E_ARG;
    return enqueue_placed(c, BatchRequest{d_bgr, width, height, row_stride, frame_stride, n_frames, grey_in_place, prev, prev_counts, false,
                                          c->input_format, 3},
                          stream);
}

extern "C" int ocvar_hip_enqueue_tracked(OcvarHip* c, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride,
                                         int n_frames, int grey_in_place, const OcvarMarker* d_prev, const int* d_prev_counts, void* stream) {
    if (!c || !d_prev || !d_prev_counts) return OCVAR_E_ARG;
    return enqueue_placed(c, BatchRequest{d_bgr, width, height, row_stride, frame_stride, n_frames, grey_in_place, d_prev, d_prev_counts,
                                          true, c->input_format, 3},
                          stream);
}

// Work that follows the batch in flight (a results copy, the overlays, the patches) is put between follow_begin and follow_end.
//
// follow_begin: the stream it goes to, ordered behind the batch.  For a batch on a lane the context's own stream means the lane,
// as NULL does: that is where the batch is, and there the work follows it without a wait.  (On the context's stream it would
// need a wait for the batch's last event -- a barrier in a hardware queue that stream shares with a lane, which holds up the
// other contexts' batches queued there until this one has finished: bench.py's multi-rank path lost a sixth of its rate to it.)
// Any other stream the caller names waits for the batch's last event.
int ocvar::follow_begin(OcvarHip* c, void* stream, hipStream_t* s) {
    *s = (!stream || (c->on_lane && (hipStream_t)stream == c->stream)) ? c->last_stream : (hipStream_t)stream;
    if (*s != c->last_stream) HIP_TRY(c, hipStreamWaitEvent(*s, c->ev[EV_LAST], 0));
    return OCVAR_OK;
}

// follow_end: behind work put on a lane collect waits for it too (it waits for events there; in front of the lanes collect's
// wait for the batch's stream covered a results copy, and bench.py's gather reads the block right after collect).
int ocvar::follow_end(OcvarHip* c, hipStream_t s) {
    if (!c->on_lane || s != c->last_stream) return OCVAR_OK;
    HIP_TRY(c, c->copied.ensure(hipEventDisableTiming));
    c->copy_pending = true;
    HIP_TRY(c, hipEventRecord(c->copied, s));
    return OCVAR_OK;
}

// what the entry points that work on the frames of the batch in flight refuse alike: no batch, or frames of another size
bool ocvar::batch_frames_ok(OcvarHip* c, const char* who, int width, int height) {
    if (!c->pending) c->err = std::string(who) + ": nothing enqueued";
    else if (width != c->ws.W || height != c->ws.H) c->err = std::string(who) + ": the frames are not of the batch's size";
    else return true;
    return false;
}

extern "C" int ocvar_hip_results_to_device(OcvarHip* c, OcvarMarker* d_markers, int* d_counts, void* stream) {
    return ocvar_hip_results_to_device_ex(c, d_markers, d_counts, c ? c->ws.maxm : MAXM, stream);
}

extern "C" int ocvar_hip_results_to_device_ex(OcvarHip* c, OcvarMarker* d_markers, int* d_counts, int max_per_frame, void* stream) {
    if (!c || !d_markers || !d_counts || !c->pending || max_per_frame < 1 || max_per_frame > c->ws.maxm) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if (int rc = follow_begin(c, stream, &s)) return rc;
    HIP_TRY(c, copy_markers(c->ws, d_markers, max_per_frame, max_per_frame, hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_counts, c->ws.n_markers, c->ws.n_frames * sizeof(int), hipMemcpyDeviceToDevice, s));
    return follow_end(c, s);
}

extern "C" int ocvar_hip_collect(OcvarHip* c, OcvarMarker* markers, int* counts, int max_per_frame) {
    if (!c || !counts || max_per_frame < 0 || (max_per_frame > 0 && !markers)) return OCVAR_E_ARG;
    if (c->board_out_off == 0) c->board_out_valid = false;
    int rc = wait_impl(c);
    if (rc) return rc;
    const int n = c->ws.n_frames;
    if (c->batch_board) {   // (a detect_host call gathers the poses of all its sub-batches)
        const size_t off = (size_t)c->board_out_off;
        if (off == 0 || c->board_out_valid) {
            c->board_out.resize(off + n);
            std::memcpy(c->board_out.data() + off, c->h_board_poses, n * sizeof(BoardPose));
            c->board_out_valid = true;
        }
    } else {
        c->board_out_valid = false;
    }
    for (int f = 0; f < n; f++) {
        counts[f] = c->h_counts[f];
        int k = counts[f] < max_per_frame ? counts[f] : max_per_frame;
        if (k > c->result_limit) k = c->result_limit;
        if (k > 0) std::memcpy(markers + (size_t)f * max_per_frame, c->h_markers + (size_t)f * c->ws.maxm, k * sizeof(OcvarMarker));
    }
    return OCVAR_OK;
}

extern "C" int ocvar_hip_ready(OcvarHip* c) {
    if (!c || !c->pending) return OCVAR_E_ARG;
    const hipError_t e = hipEventQuery(c->on_lane && c->copy_pending ? c->copied : c->ev[EV_LAST]);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        return 0;
    }
    c->err = std::string("hipEventQuery: ") + hipGetErrorString(e);
    return OCVAR_E_HIP;
}

extern "C" int ocvar_hip_set_result_limit(OcvarHip* c, int max_per_frame) {
    if (!c || c->pending || max_per_frame < 1 || max_per_frame > c->ws.maxm) return OCVAR_E_ARG;
    c->result_limit = max_per_frame;
    return OCVAR_OK;
}

extern "C" int ocvar_hip_set_input_format(OcvarHip* c, int format) {
    if (!c) return OCVAR_E_ARG;
    if (format_bpp(format) == 0) {
        c->err = "unknown input format";
        return OCVAR_E_ARG;
    }
    if (int rc = refuse_if_pending(c)) return rc;
    c->input_format = format;
    return OCVAR_OK;
}

extern "C" int ocvar_hip_set_corner_refine(OcvarHip* c, int half_win, int max_iter, float eps) {
    if (!c) return OCVAR_E_ARG;
    if (half_win < 0 || half_win > OCVAR_MAX_REFINE_HALF_WIN || max_iter < 1 || max_iter > 100 || !(eps >= 0.0f) || eps > 3.0e38f) {
        c->err = "corner refinement: half_win 0..15, max_iter 1..100, eps >= 0";
        return OCVAR_E_ARG;
    }
    // (the batch in flight, if any, took its own copy into its launch arguments)
    c->refine = refine_args_make(half_win, max_iter, eps);
    return OCVAR_OK;
}

extern "C" int ocvar_hip_set_board(OcvarHip* c, const OcvarBoardMarker* markers, int n) {
    if (!c) return OCVAR_E_ARG;
    if (n < 0 || n > OCVAR_MAX_BOARD_MARKERS || (n > 0 && !markers)) {
        c->err = "ocvar_hip_set_board: n is 0 .. 256";
        return OCVAR_E_ARG;
    }
    const BoardEntry* e = reinterpret_cast<const BoardEntry*>(markers);
    const int bad = board_first_bad(e, n);
    if (bad >= 0) {
        c->err = "ocvar_hip_set_board: entry " + std::to_string(bad) +
                 ": template id outside 0..4095 or repeated, or corners not a finite convex quad of non-zero area";
        return OCVAR_E_ARG;
    }
    if (int rc = refuse_if_pending(c)) return rc;
    if (n == 0) {
        c->board_n = 0;
        return OCVAR_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->h_board_poses) {   // (the pinned block last: its presence says that all four exist)
        int rc = dev_alloc(c, &c->d_board, BOARD_MAX);
        if (!rc) rc = dev_alloc(c, &c->d_board_map, MAXT);
        if (!rc) rc = dev_alloc(c, &c->d_board_poses, (size_t)c->ws.max_batch);
        if (rc) return rc;
        HIP_TRY(c, c->h_board_poses.reserve((size_t)c->ws.max_batch * sizeof(BoardPose)));
    }
    std::vector<int> map(MAXT, -1);
    for (int i = 0; i < n; i++) map[e[i].templateId] = i;
    // (no batch is in flight: the kernel that read the old table has finished)
    HIP_TRY(c, hipMemcpy(c->d_board, e, n * sizeof(BoardEntry), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_board_map, map.data(), MAXT * sizeof(int), hipMemcpyHostToDevice));
    c->board_n = n;
    return OCVAR_OK;
}

extern "C" int ocvar_hip_board_poses(OcvarHip* c, OcvarBoardPose* poses, int n_frames) {
    if (!c || !poses) return OCVAR_E_ARG;
    if (!c->board_out_valid) {
        c->err = "ocvar_hip_board_poses: the last collected batch had no board";
        return OCVAR_E_ARG;
    }
    if (n_frames < 1 || (size_t)n_frames > c->board_out.size()) return OCVAR_E_ARG;
    std::memcpy(poses, c->board_out.data(), (size_t)n_frames * sizeof(BoardPose));
    return OCVAR_OK;
}

extern "C" int ocvar_hip_board_poses_to_device(OcvarHip* c, OcvarBoardPose* d_poses, void* stream) {
    if (!c || !d_poses || !c->pending || !c->batch_board) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if (int rc = follow_begin(c, stream, &s)) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_poses, c->d_board_poses, (size_t)c->ws.n_frames * sizeof(BoardPose), hipMemcpyDeviceToDevice, s));
    return follow_end(c, s);
}

extern "C" int ocvar_hip_detect_device(OcvarHip* c, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride,
                                       int n_frames, int grey_in_place, const OcvarMarker* prev, const int* prev_counts,
                                       OcvarMarker* markers, int* counts, int max_per_frame) {
    int rc = ocvar_hip_enqueue(c, d_bgr, width, height, row_stride, frame_stride, n_frames, grey_in_place, prev, prev_counts, nullptr);
    if (rc) return rc;
    return ocvar_hip_collect(c, markers, counts, max_per_frame);
}

extern "C" int ocvar_hip_stage_ms(OcvarHip* c, float* ms, int n) {
    if (!c || !ms || n < 1 || c->pending) return OCVAR_E_ARG;
    int k = 0;
    for (; k < EV_STAGES && k < n; k++)
        if (hipEventElapsedTime(&ms[k], c->ev[k], c->ev[k + 1]) != hipSuccess) ms[k] = -1.f;
    if (k < n && k == EV_STAGES) {   // the whole batch
        if (hipEventElapsedTime(&ms[k], c->ev[0], c->ev[EV_LAST]) != hipSuccess) ms[k] = -1.f;
        k++;
    }
    return k;
}

// Where the last batch's stage events (EV_COUNT = 13) lie on the device's clock, in milliseconds after the caller's reference event
// (recorded on any stream of this device before the batch was enqueued).  With several contexts in flight the launches of one
// kernel overlap each other; their start/end stamps let a caller compute how long the GPU was running that kernel at all.
extern "C" int ocvar_hip_stage_stamps(OcvarHip* c, void* ref_event, float* ms, int n) {
    if (!c || !ref_event || !ms || n < 1 || c->pending) return OCVAR_E_ARG;
    int k = 0;
    for (; k < EV_COUNT && k < n; k++)
        if (hipEventElapsedTime(&ms[k], (hipEvent_t)ref_event, c->ev[k]) != hipSuccess) {
            (void)hipGetLastError();
            ms[k] = -1.f;
        }
    return k;
}

extern "C" int ocvar_hip_counters(OcvarHip* c, long long* out, int n) {
    if (!c || !out || n < 1 || c->pending) return OCVAR_E_ARG;
    const int* h = c->h_counters;
    long long v[10] = {h[CNT_FRAME_CANDS], h[CNT_CROP_ROIS], h[CNT_CROP_TILES], h[CNT_CROP_CANDS],
                      (long long)*reinterpret_cast<const unsigned long long*>(h + CNT_CROP_PIXELS),
                      (long long)*reinterpret_cast<const unsigned long long*>(h + CNT_POOL_INTS),
                      h[CNT_MID_F], h[CNT_MID_C], h[CNT_LONG_F], h[CNT_LONG_C]};
    int k = 0;
    for (; k < 10 && k < n; k++) out[k] = v[k];
    // values 10..41: profiling slots (zero unless the library was built with -DOCVAR_PROF)
    for (; k < 42 && k < n; k++) out[k] = (long long)reinterpret_cast<const unsigned long long*>(h + CNT_PROF)[k - 10];
    return k;
}
