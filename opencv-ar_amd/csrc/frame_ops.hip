// frame_ops.hip -- the opt-in operations of the C ABI on frames and marker records in device memory: overlays, annotation,
// patches, undistortion, YUV conversion, resizing, turning, warping, levels, demosaic and flow tracking.  An entry point is its own
// parameter checks, the shared checks of its frame blocks (frames_core.h; here they get their error texts), and its launches in
// chunks of frames.  Every refusal (OCVAR_E_ARG and a text that begins with the operation's name) comes before any device call.
#include "context.h"
#include "frames_core.h"
#include <algorithm>
#include <new>

using namespace ocvar;

static_assert(OCVAR_FMT_BGR == 0 && OCVAR_FMT_RGB == 1 && OCVAR_FMT_BGRA == 2 && OCVAR_FMT_RGBA == 3 && OCVAR_FMT_GRAY == 4, "format_bpp's codes");

namespace {

int refuse(OcvarHip* c, const char* who, const std::string& text) {
    c->err = std::string(who) + ": " + text;
    return OCVAR_E_ARG;
}

hipStream_t stream_or_own(const OcvarHip* c, void* stream) { return stream ? (hipStream_t)stream : c->stream.s; }

// The sides an operation admits: frames the context's workspaces are sized for, or any the kernels' 16-bit coordinates hold.
struct SideLimit {
    int w, h;
};
SideLimit context_size(const OcvarHip* c) { return {c->ws.max_w, c->ws.max_h}; }
constexpr SideLimit ANY_SIZE{32767, 32767};

// One text per reason of frames_check (by FramesBad).  An operation whose text for a reason says more -- it names a parameter of
// its own in the same breath, or its sides have other limits -- takes the table `with` that text.
struct FrameTexts {
    const char* why[6];
};
constexpr FrameTexts TEXTS{{"", "an unknown format", "sides of 1 .. 32767 pixels", "n_frames >= 1",
                            "a row stride below the format's bytes per pixel times width", "the rows of a frame span more than 2147483647 bytes"}};
constexpr FrameTexts with(FrameTexts t, int reason, const char* text) {
    t.why[reason] = text;
    return t;
}
// (frames bound by the context's size: sides and count share a text)
constexpr FrameTexts context_texts(const char* size_text) { return with(with(TEXTS, FRAMES_SIDE, size_text), FRAMES_COUNT, size_text); }

FrameBlock block_of(const uint8_t* p, int width, int height, int bpp, int row_stride, size_t frame_stride, int n_frames) {
    return FrameBlock{p, width, height, bpp, row_stride, frame_stride, n_frames};
}

// One block: format, sides, n_frames, row stride and -- with span_rule -- the rows' span.  (Without: the operations whose
// kernels address rows by 64-bit offsets, and those that apply frame_span_check, the binarise kernel's rule.)
int block_check(OcvarHip* c, const char* who, const FrameBlock& b, const SideLimit& lim, const FrameTexts& texts, bool span_rule) {
    const int bad = frames_check(b, lim.w, lim.h);
    if (bad == FRAMES_OK || (bad == FRAMES_SPAN && !span_rule)) return OCVAR_OK;
    return refuse(c, who, texts.why[bad]);
}

// A source block, a destination block, and that they share no byte (`verb`: what the operation does not do in place; `sides`:
// what it calls the two).
int pair_check(OcvarHip* c, const char* who, const FrameBlock& src, const FrameBlock& dst, const SideLimit& lim, const FrameTexts& texts,
               const char* verb, bool span_rule = true, const char* sides = "source and destination frames") {
    if (int rc = block_check(c, who, src, lim, texts, span_rule)) return rc;
    if (int rc = block_check(c, who, dst, lim, texts, span_rule)) return rc;
    if (!frames_intersect(src, dst)) return OCVAR_OK;
    return refuse(c, who, std::string("the byte ranges of ") + sides + " intersect (no " + verb + " in place)");
}

// n_frames frames on stream s in chunks: launch(f0, n) puts frames f0 .. f0 + n - 1 there.
template <typename Launch>
int run_chunks(OcvarHip* c, const char* what, int n_frames, int chunk, hipStream_t s, Launch launch) {
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        launch(f0, std::min(chunk, n_frames - f0));
        TRACE_LAUNCH(what, s);
    }
    HIP_TRY(c, hipGetLastError());
    return OCVAR_OK;
}

constexpr int GRID_Z_HALF = 32768;   // frames as the grid's z of a kernel pair that shares a batch-sized workspace
constexpr int GRID_Z = 65535;

// What the *_records entry points refuse alike, and their launches: records_run comes behind the operation's own checks.
int records_check(OcvarHip* c, const char* who, bool pointers, int n_frames, int records_per_frame,
                  const char* no_pointers = "no records, no counts or no output") {
    if (!pointers) return refuse(c, who, no_pointers);
    if (n_frames < 1 || records_per_frame < 1 || records_per_frame > c->ws.maxm) return refuse(c, who, "n_frames >= 1, 1 .. M records per frame");
    return OCVAR_OK;
}
template <typename Launch>
int records_run(OcvarHip* c, const char* who, int n_frames, void* stream, Launch launch) {
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    return run_chunks(c, who, n_frames, GRID_Z, s, [&](int f0, int n) { launch(f0, n, s); });
}
const MarkerRec* recs_at(const OcvarMarker* m, int f0, int per_frame) { return reinterpret_cast<const MarkerRec*>(m) + (size_t)f0 * per_frame; }
MarkerRec* recs_at(OcvarMarker* m, int f0, int per_frame) { return reinterpret_cast<MarkerRec*>(m) + (size_t)f0 * per_frame; }

// What the entry points that draw or cut with the records of the batch in flight (`who`), or with records the caller names
// (`who`_records: then of n_frames frames of up to the context's size), refuse alike of their frames: a format and a row stride.
int drawn_frames_check(OcvarHip* c, const char* who, const char* no_frames, const char* format_or_stride, const uint8_t* d_frames, int width,
                       int height, int row_stride, size_t frame_stride, int n_frames, int format) {
    if (!d_frames) return refuse(c, who, no_frames);
    const FrameTexts texts = with(with(TEXTS, FRAMES_FORMAT, format_or_stride), FRAMES_ROW_STRIDE, format_or_stride);
    return block_check(c, who, block_of(d_frames, width, height, format_bpp(format), row_stride, frame_stride, n_frames), context_size(c), texts, false);
}
// ... and what the `who`_records ones refuse before that, under one text
bool drawn_records_ok(const OcvarHip* c, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int width, int height) {
    return d_markers && d_counts && n_frames >= 1 && width >= 1 && height >= 1 && width <= c->ws.max_w && height <= c->ws.max_h;
}
bool per_frame_ok(const OcvarHip* c, int records_per_frame) { return records_per_frame >= 1 && records_per_frame <= c->ws.maxm; }
constexpr const char* DRAWN_FRAMES = "no frames, an unknown format or a row_stride below the format's bytes per pixel times width";
constexpr const char* DRAWN_RECORDS = "frames of 1 .. the context's size, n_frames >= 1, 1 .. M records per frame";

}  // namespace

extern "C" int ocvar_hip_set_overlay(OcvarHip* c, int template_id, const uint8_t* h_rgba, int width, int height, int row_stride) {
    if (!c) return OCVAR_E_ARG;
    if (template_id < -1 || template_id >= MAXT) return refuse(c, "ocvar_hip_set_overlay", "template id outside -1 .. 4095");
    if (h_rgba && (width < 2 || height < 2 || width > OVL_MAX_SIDE || height > OVL_MAX_SIDE || (long long)row_stride < 4ll * width))
        return refuse(c, "ocvar_hip_set_overlay", "sides 2 .. 1024 texels, row_stride >= 4 width");
    if (int rc = refuse_if_pending(c)) return rc;
    OverlayTable* t = c->h_overlays;
    int slot = !t ? -1 : (template_id < 0 ? t->dflt : t->map[template_id]);
    if (!h_rgba && slot < 0) return OCVAR_OK;   // (nothing to remove)
    if (h_rgba && slot < 0 && c->n_overlays >= OVL_MAX) return refuse(c, "ocvar_hip_set_overlay", "the context has OCVAR_MAX_OVERLAYS overlays");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!t) {   // (the host table last: its presence says that the device blocks exist)
        const size_t recs = (size_t)c->ws.max_batch * c->ws.maxm;
        int rc = dev_alloc(c, &c->d_overlays, 1);
        if (!rc) rc = dev_alloc(c, &c->d_ovl_draws, recs);
        if (!rc) rc = dev_alloc(c, &c->d_ovl_boxes, recs);
        if (rc) return rc;
        t = new (std::nothrow) OverlayTable();
        if (!t) return OCVAR_E_HIP;
        for (auto& x : t->tex) x = OverlayTex{nullptr, 0, 0};
        t->dflt = -1;
        for (auto& m : t->map) m = -1;
        c->h_overlays = t;
    }
    HIP_TRY(c, c->ovl_fence.drain());   // (a render_records in flight reads the table and the images)
    if (slot >= 0) {   // removed, or replaced below
        HIP_TRY(c, hipFree(const_cast<uint32_t*>(t->tex[slot].px)));
        t->tex[slot] = OverlayTex{nullptr, 0, 0};
        (template_id < 0 ? t->dflt : t->map[template_id]) = -1;
        c->n_overlays--;
    }
    if (h_rgba) {
        for (slot = 0; slot < OVL_MAX && t->tex[slot].px; slot++) {}
        void* d = nullptr;
        HIP_TRY(c, hipMalloc(&d, (size_t)width * height * 4));
        const hipError_t e = hipMemcpy2D(d, (size_t)width * 4, h_rgba, (size_t)row_stride, (size_t)width * 4, (size_t)height, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            c->err = std::string("ocvar_hip_set_overlay: ") + hipGetErrorString(e);
            return OCVAR_E_HIP;
        }
        t->tex[slot] = OverlayTex{static_cast<const uint32_t*>(d), width, height};
        (template_id < 0 ? t->dflt : t->map[template_id]) = slot;
        c->n_overlays++;
    }
    HIP_TRY(c, hipMemcpy(c->d_overlays, t, sizeof(OverlayTable), hipMemcpyHostToDevice));
    return OCVAR_OK;
}

// setup + draw of n_frames frames (chunks of the workspace's max_batch) on stream s, behind the workspace's last use
static int overlay_launch(OcvarHip* c, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int n_frames,
                          int format, const MarkerRec* recs, const int* counts, int stride, hipStream_t s) {
    HIP_TRY(c, c->ovl_fence.enter(s));
    const OverlayArgs oa{c->d_overlays, c->d_ovl_draws, c->d_ovl_boxes};
    const int rc = run_chunks(c, "overlay", n_frames, std::min(c->ws.max_batch, GRID_Z_HALF), s, [&](int f0, int n) {
        launch_overlay(oa, d_frames + (size_t)f0 * frame_stride, width, height, row_stride, (long long)frame_stride, n, format,
                       recs + (size_t)f0 * stride, counts + f0, stride, s);
    });
    if (rc) return rc;
    HIP_TRY(c, c->ovl_fence.leave(s));
    return OCVAR_OK;
}

extern "C" int ocvar_hip_render(OcvarHip* c, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int format,
                                void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!batch_frames_ok(c, "render", width, height)) return OCVAR_E_ARG;
    if (int rc = drawn_frames_check(c, "render", DRAWN_FRAMES, DRAWN_FRAMES, d_frames, width, height, row_stride, frame_stride, c->ws.n_frames, format)) return rc;
    if (c->n_overlays < 1) return refuse(c, "render", "no overlay is set");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if (int rc = follow_begin(c, stream, &s)) return rc;
    const int rc = overlay_launch(c, d_frames, width, height, row_stride, frame_stride, c->ws.n_frames, format, c->ws.markers,
                                  c->ws.n_markers, c->ws.maxm, s);
    if (rc) return rc;
    return follow_end(c, s);
}

extern "C" int ocvar_hip_render_records(OcvarHip* c, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride,
                                        int n_frames, int format, const OcvarMarker* d_markers, const int* d_counts,
                                        int records_per_frame, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!drawn_records_ok(c, d_markers, d_counts, n_frames, width, height) || !per_frame_ok(c, records_per_frame)) return refuse(c, "render_records", DRAWN_RECORDS);
    if (int rc = drawn_frames_check(c, "render", DRAWN_FRAMES, DRAWN_FRAMES, d_frames, width, height, row_stride, frame_stride, n_frames, format)) return rc;
    if (c->n_overlays < 1) return refuse(c, "render", "no overlay is set");
    HIP_TRY(c, hipSetDevice(c->device));
    return overlay_launch(c, d_frames, width, height, row_stride, frame_stride, n_frames, format, recs_at(d_markers, 0, 0), d_counts,
                          records_per_frame, stream_or_own(c, stream));
}

extern "C" int ocvar_hip_annotate_default_style(OcvarAnnotateStyle* style) {
    if (!style) return OCVAR_E_ARG;
    anno_default_style(style);
    return OCVAR_OK;
}

static int annotate_style_check(OcvarHip* c, const char* who, const OcvarAnnotateStyle* style) {
    static const char* const why[] = {"", "no style", "thickness 1 .. 16", "label_scale 0 .. 8", "axis_length and cube_height are finite numbers >= 0",
                                      "unknown flag bits", "none of OUTLINE, CORNER0, AXES, CUBE and LABEL is set", "AXES or CUBE without a camera"};
    const int bad = anno_style_bad(style, c->have_camera);
    return bad ? refuse(c, who, why[bad]) : OCVAR_OK;
}

// setup + draw of n_frames frames (chunks of the workspace's max_batch) on stream s, behind the workspace's last use
static int annotate_launch(OcvarHip* c, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int n_frames,
                           int format, const MarkerRec* recs, const int* counts, int stride, const OcvarAnnotateStyle& st, hipStream_t s) {
    const size_t slots = (size_t)c->ws.max_batch * c->ws.maxm;
    HIP_TRY(c, c->anno_recs.reserve(slots * sizeof(AnnoRec)));
    HIP_TRY(c, c->anno_boxes.reserve(slots * sizeof(AnnoBox)));
    HIP_TRY(c, c->anno_fence.enter(s));
    const AnnoArgs aa{c->anno_recs, c->anno_boxes};
    const int rc = run_chunks(c, "annotate", n_frames, std::min(c->ws.max_batch, GRID_Z_HALF), s, [&](int f0, int n) {
        launch_annotate(aa, d_frames + (size_t)f0 * frame_stride, width, height, row_stride, (long long)frame_stride, n, format,
                        recs + (size_t)f0 * stride, counts + f0, stride, st, c->h_camera, s);
    });
    if (rc) return rc;
    HIP_TRY(c, c->anno_fence.leave(s));
    return OCVAR_OK;
}

extern "C" int ocvar_hip_annotate(OcvarHip* c, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int format,
                                  const OcvarAnnotateStyle* style, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!batch_frames_ok(c, "annotate", width, height)) return OCVAR_E_ARG;
    if (int rc = drawn_frames_check(c, "annotate", DRAWN_FRAMES, DRAWN_FRAMES, d_frames, width, height, row_stride, frame_stride, c->ws.n_frames, format)) return rc;
    if (int rc = annotate_style_check(c, "annotate", style)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if (int rc = follow_begin(c, stream, &s)) return rc;
    const int rc = annotate_launch(c, d_frames, width, height, row_stride, frame_stride, c->ws.n_frames, format, c->ws.markers,
                                   c->ws.n_markers, c->ws.maxm, *style, s);
    if (rc) return rc;
    return follow_end(c, s);
}

extern "C" int ocvar_hip_annotate_records(OcvarHip* c, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride,
                                          int n_frames, int format, const OcvarMarker* d_markers, const int* d_counts,
                                          int records_per_frame, const OcvarAnnotateStyle* style, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!drawn_records_ok(c, d_markers, d_counts, n_frames, width, height) || !per_frame_ok(c, records_per_frame)) return refuse(c, "annotate_records", DRAWN_RECORDS);
    if (int rc = drawn_frames_check(c, "annotate", DRAWN_FRAMES, DRAWN_FRAMES, d_frames, width, height, row_stride, frame_stride, n_frames, format)) return rc;
    if (int rc = annotate_style_check(c, "annotate", style)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return annotate_launch(c, d_frames, width, height, row_stride, frame_stride, n_frames, format, recs_at(d_markers, 0, 0), d_counts,
                           records_per_frame, *style, stream_or_own(c, stream));
}

// what ocvar_hip_patches and ocvar_hip_patches_records refuse alike, of the frames and of the patches
constexpr const char* PATCH_POINTERS = "no frames or no patch buffer";
static int patch_args_check(OcvarHip* c, const uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int n_frames, int format,
                            const uint8_t* d_patches, int patch_w, int patch_h, int records_per_frame, int flags) {
    const char* const who = "patches";
    if (!d_patches) return refuse(c, who, PATCH_POINTERS);
    if (int rc = drawn_frames_check(c, who, PATCH_POINTERS, "an unknown format or a row_stride below the format's bytes per pixel times width", d_frames,
                                    width, height, row_stride, frame_stride, n_frames, format))
        return rc;
    if (patch_w < 2 || patch_h < 2 || patch_w > PATCH_MAX_SIDE || patch_h > PATCH_MAX_SIDE)
        return refuse(c, who, "patch sides of 2 .. " + std::to_string(PATCH_MAX_SIDE) + " pixels");
    if (flags & ~PATCH_FLAGS) return refuse(c, who, "unknown flag bits");
    if (!per_frame_ok(c, records_per_frame)) return refuse(c, who, "1 .. M records per frame");
    return OCVAR_OK;
}

// n_frames frames on stream s, in chunks of the grid's z
static int patch_launch(OcvarHip* c, const PatchArgs& all, int n_frames, int format, hipStream_t s) {
    const size_t frame_patches = (size_t)all.slots * all.ph * all.pw * format_bpp(format);
    return run_chunks(c, "patches", n_frames, GRID_Z_HALF, s, [&](int f0, int n) {
        PatchArgs a = all;
        a.frames += (size_t)f0 * a.frame_stride;
        a.recs += (size_t)f0 * a.rec_stride;
        a.counts += f0;
        a.patches += (size_t)f0 * frame_patches;
        if (a.status) a.status += (size_t)f0 * a.slots;
        launch_patches(a, n, format, s);
    });
}

extern "C" int ocvar_hip_patches(OcvarHip* c, const uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int format,
                                 uint8_t* d_patches, int patch_w, int patch_h, int records_per_frame, int flags, int* d_status, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!batch_frames_ok(c, "patches", width, height)) return OCVAR_E_ARG;
    if (int rc = patch_args_check(c, d_frames, width, height, row_stride, frame_stride, c->ws.n_frames, format, d_patches, patch_w, patch_h, records_per_frame, flags))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s;
    if (int rc = follow_begin(c, stream, &s)) return rc;
    const PatchArgs a{d_frames, width, height, (long long)row_stride, (long long)frame_stride, c->ws.markers, c->ws.n_markers, c->ws.maxm,
                      d_patches, patch_w, patch_h, records_per_frame, flags, d_status};
    const int rc = patch_launch(c, a, c->ws.n_frames, format, s);
    if (rc) return rc;
    return follow_end(c, s);
}

extern "C" int ocvar_hip_patches_records(OcvarHip* c, const uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride,
                                         int n_frames, int format, const OcvarMarker* d_markers, const int* d_counts, int records_per_frame,
                                         uint8_t* d_patches, int patch_w, int patch_h, int flags, int* d_status, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!drawn_records_ok(c, d_markers, d_counts, n_frames, width, height))
        return refuse(c, "patches_records", "records and counts, frames of 1 .. the context's size, n_frames >= 1");
    if (int rc = patch_args_check(c, d_frames, width, height, row_stride, frame_stride, n_frames, format, d_patches, patch_w, patch_h, records_per_frame, flags))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const PatchArgs a{d_frames, width, height, (long long)row_stride, (long long)frame_stride, recs_at(d_markers, 0, 0), d_counts,
                      records_per_frame, d_patches, patch_w, patch_h, records_per_frame, flags, d_status};
    return patch_launch(c, a, n_frames, format, stream_or_own(c, stream));
}

// the context's camera as the undistort entry points take it; refused when there is none they can use
static int undistort_camera(OcvarHip* c, const char* who, UndistortCam* cam) {
    if (!c->have_camera) return refuse(c, who, "no camera set");
    *cam = undistort_cam(c->h_camera);
    if (undistort_cam_ok(*cam)) return OCVAR_OK;
    return refuse(c, who, "the camera's fx or fy is zero, or one of fx fy cx cy k1 k2 p1 p2 k3 is not finite");
}

extern "C" int ocvar_hip_undistort(OcvarHip* c, const uint8_t* d_src, int src_row_stride, size_t src_frame_stride, uint8_t* d_dst,
                                   int dst_row_stride, size_t dst_frame_stride, int width, int height, int n_frames, int format, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!d_src || !d_dst) return refuse(c, "undistort", "no source or no destination frames");
    const int bpp = format_bpp(format);
    // (the rows' span by the binarise kernel's rule, as for the frames of a batch: it rounds the sides down to even)
    const FrameBlock src = block_of(d_src, width, height, bpp, src_row_stride, src_frame_stride, n_frames);
    const FrameBlock dst = block_of(d_dst, width, height, bpp, dst_row_stride, dst_frame_stride, n_frames);
    constexpr const char* FORMAT_OR_STRIDE = "an unknown format or a row stride below the format's bytes per pixel times width";
    constexpr FrameTexts texts = with(with(context_texts("frames of 1 .. the context's size, n_frames >= 1"), FRAMES_FORMAT, FORMAT_OR_STRIDE),
                                      FRAMES_ROW_STRIDE, FORMAT_OR_STRIDE);
    if (int rc = block_check(c, "undistort", src, context_size(c), texts, false)) return rc;
    if (int rc = block_check(c, "undistort", dst, context_size(c), texts, false)) return rc;
    if (int rc = frame_span_check(c, width, height, src_row_stride, format)) return rc;
    if (int rc = frame_span_check(c, width, height, dst_row_stride, format)) return rc;
    if (int rc = pair_check(c, "undistort", src, dst, context_size(c), texts, "undistortion", false)) return rc;   // (the blocks hold: the ranges)
    UndistortCam cam;
    if (int rc = undistort_camera(c, "undistort", &cam)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    return run_chunks(c, "undistort", n_frames, GRID_Z, s, [&](int f0, int n) {
        const UndistortArgs a{d_src + (size_t)f0 * src_frame_stride, d_dst + (size_t)f0 * dst_frame_stride, width, height,
                              (long long)src_row_stride, (long long)src_frame_stride, (long long)dst_row_stride, (long long)dst_frame_stride, cam};
        launch_undistort(a, n, format, s);
    });
}

extern "C" int ocvar_hip_undistort_records(OcvarHip* c, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int records_per_frame,
                                           OcvarMarker* d_out, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (int rc = records_check(c, "undistort_records", d_markers && d_counts && d_out, n_frames, records_per_frame)) return rc;
    UndistortCam cam;
    if (int rc = undistort_camera(c, "undistort_records", &cam)) return rc;
    return records_run(c, "undistort_records", n_frames, stream, [&](int f0, int n, hipStream_t s) {
        launch_undistort_records(UndistortRecArgs{recs_at(d_markers, f0, records_per_frame), recs_at(d_out, f0, records_per_frame), d_counts + f0,
                                                  records_per_frame, cam}, n, s);
    });
}

// What ocvar_hip_yuv_to_frames and ocvar_hip_frames_to_yuv refuse alike, and the launches: yuv describes one side, pix the other.
static int yuv_convert(OcvarHip* c, const char* who, const OcvarYuvFrames* yuv, const uint8_t* pix, int row_stride, size_t frame_stride,
                       int width, int height, int n_frames, int format, bool to_frames, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!yuv || !pix) return refuse(c, who, "no YUV frames or no frames");
    constexpr const char* UNKNOWN = "an unknown layout, matrix or format";
    constexpr FrameTexts texts = with(with(context_texts("frames of 1 .. the context's size, n_frames >= 1"), FRAMES_FORMAT, UNKNOWN), FRAMES_SPAN,
                                      "the rows of a plane or of a frame span more than 2147483647 bytes");
    if (!yuv_layout_ok(yuv->layout) || !yuv_matrix_ok(yuv->matrix)) return refuse(c, who, UNKNOWN);
    const bool s420 = yuv_is_420(yuv->layout);
    if (!yuv->y || (s420 && !yuv->c0) || (yuv->layout == OCVAR_YUV_I420 && !yuv->c1)) return refuse(c, who, "a plane the layout uses is NULL");
    const SideLimit lim = context_size(c);
    const FrameBlock frames = block_of(pix, width, height, format_bpp(format), row_stride, frame_stride, n_frames);
    if (int rc = block_check(c, who, frames, lim, texts, true)) return rc;
    if ((width & 1) || (s420 && (height & 1))) return refuse(c, who, "an odd width, or an odd height with NV12 or I420");
    // the planes as blocks of bytes: a packed row has two bytes per pixel
    FrameBlock planes[3];
    int n_planes = 0;
    planes[n_planes++] = block_of(yuv->y, s420 ? width : 2 * width, height, 1, yuv->y_pitch, yuv->frame_stride, n_frames);
    if (yuv->layout == OCVAR_YUV_NV12) planes[n_planes++] = block_of(yuv->c0, width, height / 2, 1, yuv->c_pitch, yuv->frame_stride, n_frames);
    if (yuv->layout == OCVAR_YUV_I420) {
        planes[n_planes++] = block_of(yuv->c0, width / 2, height / 2, 1, yuv->c_pitch, yuv->frame_stride, n_frames);
        planes[n_planes++] = block_of(yuv->c1, width / 2, height / 2, 1, yuv->c_pitch, yuv->frame_stride, n_frames);
    }
    const SideLimit plane_lim{2 * lim.w, lim.h};
    for (int i = 0; i < n_planes; i++) {
        if (planes[i].row_stride < planes[i].width) return refuse(c, who, "a pitch below the plane's bytes per row");
        if (int rc = pair_check(c, who, planes[i], frames, plane_lim, texts, "conversion", true, "a YUV plane and of the frames")) return rc;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    return run_chunks(c, who, n_frames, YUV_CHUNK_FRAMES, s, [&](int f0, int n) {
        const size_t yo = (size_t)f0 * yuv->frame_stride;
        const YuvArgs a{yuv->y + yo, yuv->c0 ? yuv->c0 + yo : nullptr, yuv->c1 ? yuv->c1 + yo : nullptr, (long long)yuv->y_pitch,
                        (long long)yuv->c_pitch, (long long)yuv->frame_stride, const_cast<uint8_t*>(pix) + (size_t)f0 * frame_stride,
                        (long long)row_stride, (long long)frame_stride, width, height, yuv->layout, format, yuv_coef(yuv->matrix)};
        launch_yuv(a, n, to_frames, s);
    });
}

extern "C" int ocvar_hip_yuv_to_frames(OcvarHip* c, const OcvarYuvFrames* src, uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride,
                                       int width, int height, int n_frames, int format, void* stream) {
    return yuv_convert(c, "yuv_to_frames", src, d_dst, dst_row_stride, dst_frame_stride, width, height, n_frames, format, true, stream);
}

extern "C" int ocvar_hip_frames_to_yuv(OcvarHip* c, const uint8_t* d_src, int src_row_stride, size_t src_frame_stride, const OcvarYuvFrames* dst,
                                       int width, int height, int n_frames, int format, void* stream) {
    return yuv_convert(c, "frames_to_yuv", dst, d_src, src_row_stride, src_frame_stride, width, height, n_frames, format, false, stream);
}

// What ocvar_hip_yuv_to_frames_ex and ocvar_hip_frames_to_yuv_ex refuse alike (yuv_ex_core.h::yuv_ex_check: here the reasons get
// their texts), and the launches.
static int yuv_ex_convert(OcvarHip* c, const char* who, const OcvarYuvFramesEx* yuv, const uint8_t* pix, int row_stride, size_t frame_stride,
                          int width, int height, int n_frames, int format, bool to_frames, void* stream) {
    if (!c) return OCVAR_E_ARG;
    static const char* const why[] = {"", "no YUV frames or no frames", "an unknown layout, matrix, range, bits or format",
                                      "more than 8 bits with a layout other than NV12", "a plane the layout uses is NULL",
                                      "frames of 1 .. the context's size, n_frames >= 1", "a row stride below the format's bytes per pixel times width",
                                      "the rows of a plane or of a frame span more than 2147483647 bytes",
                                      "an odd width with a layout that halves it, or an odd height with NV12, NV21 or I420",
                                      "16-bit samples at an odd address, pitch or frame stride", "a pitch below the plane's bytes per row",
                                      "the byte ranges of a YUV plane and of the frames intersect (no conversion in place)"};
    static_assert(sizeof(why) / sizeof(why[0]) == YUV_EX_OVERLAP + 1, "one text per reason of yuv_ex_check");
    const SideLimit lim = context_size(c);
    if (int bad = yuv_ex_check(yuv, pix, row_stride, frame_stride, width, height, n_frames, format, lim.w, lim.h)) return refuse(c, who, why[bad]);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    return run_chunks(c, who, n_frames, YUV_CHUNK_FRAMES, s, [&](int f0, int n) {
        launch_yuv_ex(yuv_ex_args(*yuv, (size_t)f0, pix, row_stride, frame_stride, width, height, format), n, to_frames, s);
    });
}

extern "C" int ocvar_hip_yuv_to_frames_ex(OcvarHip* c, const OcvarYuvFramesEx* src, uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride,
                                          int width, int height, int n_frames, int format, void* stream) {
    return yuv_ex_convert(c, "yuv_to_frames_ex", src, d_dst, dst_row_stride, dst_frame_stride, width, height, n_frames, format, true, stream);
}

extern "C" int ocvar_hip_frames_to_yuv_ex(OcvarHip* c, const uint8_t* d_src, int src_row_stride, size_t src_frame_stride, const OcvarYuvFramesEx* dst,
                                          int width, int height, int n_frames, int format, void* stream) {
    return yuv_ex_convert(c, "frames_to_yuv_ex", dst, d_src, src_row_stride, src_frame_stride, width, height, n_frames, format, false, stream);
}

extern "C" int ocvar_hip_resize(OcvarHip* c, const uint8_t* d_src, int src_width, int src_height, int src_row_stride, size_t src_frame_stride,
                                uint8_t* d_dst, int dst_width, int dst_height, int dst_row_stride, size_t dst_frame_stride, int n_frames,
                                int format, int interpolation, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!d_src || !d_dst) return refuse(c, "resize", "no source or no destination frames");
    constexpr FrameTexts texts = with(TEXTS, FRAMES_FORMAT, "an unknown format or interpolation");
    if (!resize_interp_ok(interpolation)) return refuse(c, "resize", texts.why[FRAMES_FORMAT]);
    const int bpp = format_bpp(format);
    if (int rc = pair_check(c, "resize", block_of(d_src, src_width, src_height, bpp, src_row_stride, src_frame_stride, n_frames),
                            block_of(d_dst, dst_width, dst_height, bpp, dst_row_stride, dst_frame_stride, n_frames), ANY_SIZE, texts, "resizing"))
        return rc;
    if (interpolation == OCVAR_RESIZE_AREA && !resize_area_ok(src_width, src_height, dst_width, dst_height))
        return refuse(c, "resize", "AREA shrinks only, by at most OCVAR_MAX_RESIZE_RATIO per axis");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    const ResizePlan plan = resize_plan(src_width, src_height, dst_width, dst_height, interpolation);
    return run_chunks(c, "resize", n_frames, RESIZE_CHUNK_FRAMES, s, [&](int f0, int n) {
        const ResizeArgs a{d_src + (size_t)f0 * src_frame_stride, d_dst + (size_t)f0 * dst_frame_stride, src_width, src_height, dst_width, dst_height,
                           (long long)src_row_stride, (long long)src_frame_stride, (long long)dst_row_stride, (long long)dst_frame_stride, plan};
        launch_resize(a, n, format, s);
    });
}

static bool any_size_ok(int width, int height) { return width >= 1 && width <= ANY_SIZE.w && height >= 1 && height <= ANY_SIZE.h; }

extern "C" int ocvar_hip_scale_records(OcvarHip* c, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int records_per_frame,
                                       int src_width, int src_height, int dst_width, int dst_height, int flags, OcvarMarker* d_out, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (int rc = records_check(c, "scale_records", d_markers && d_counts && d_out, n_frames, records_per_frame)) return rc;
    if (!any_size_ok(src_width, src_height) || !any_size_ok(dst_width, dst_height)) return refuse(c, "scale_records", TEXTS.why[FRAMES_SIDE]);
    if (flags & ~RESIZE_FLAGS) return refuse(c, "scale_records", "unknown flag bits");
    if ((flags & OCVAR_SCALE_POSE) && !c->have_camera) return refuse(c, "scale_records", "OCVAR_SCALE_POSE without a camera");
    return records_run(c, "scale_records", n_frames, stream, [&](int f0, int n, hipStream_t s) {
        launch_scale_records(ScaleRecArgs{recs_at(d_markers, f0, records_per_frame), recs_at(d_out, f0, records_per_frame), d_counts + f0,
                                          records_per_frame, src_width, src_height, dst_width, dst_height, flags, c->h_camera}, n, s);
    });
}

extern "C" int ocvar_hip_orient(OcvarHip* c, const uint8_t* d_src, int src_width, int src_height, int src_row_stride, size_t src_frame_stride,
                                uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride, int n_frames, int format, int orientation, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!d_src || !d_dst) return refuse(c, "orient", "no source or no destination frames");
    constexpr FrameTexts texts = with(with(TEXTS, FRAMES_FORMAT, "an unknown format or orientation"), FRAMES_ROW_STRIDE,
                                      "a row stride below the format's bytes per pixel times the width of that side");
    if (!orient_ok(orientation)) return refuse(c, "orient", texts.why[FRAMES_FORMAT]);
    const int bpp = format_bpp(format);
    const int dst_width = orient_dst_width(orientation, src_width, src_height), dst_height = orient_dst_height(orientation, src_width, src_height);
    if (int rc = pair_check(c, "orient", block_of(d_src, src_width, src_height, bpp, src_row_stride, src_frame_stride, n_frames),
                            block_of(d_dst, dst_width, dst_height, bpp, dst_row_stride, dst_frame_stride, n_frames), ANY_SIZE, texts, "turning"))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    return run_chunks(c, "orient", n_frames, ORIENT_CHUNK_FRAMES, s, [&](int f0, int n) {
        const OrientArgs a{d_src + (size_t)f0 * src_frame_stride, d_dst + (size_t)f0 * dst_frame_stride, src_width, src_height,
                           (long long)src_row_stride, (long long)src_frame_stride, (long long)dst_row_stride, (long long)dst_frame_stride, orientation};
        launch_orient(a, n, format, s);
    });
}

extern "C" int ocvar_hip_orient_records(OcvarHip* c, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int records_per_frame,
                                        int src_width, int src_height, int orientation, int flags, OcvarMarker* d_out, void* stream) {
    if (!c) return OCVAR_E_ARG;
    const char* const who = "orient_records";
    if (int rc = records_check(c, who, d_markers && d_counts && d_out, n_frames, records_per_frame)) return rc;
    if (!any_size_ok(src_width, src_height)) return refuse(c, who, TEXTS.why[FRAMES_SIDE]);
    if (!orient_ok(orientation)) return refuse(c, who, "an unknown orientation");
    if (flags & ~ORIENT_FLAGS) return refuse(c, who, "unknown flag bits");
    if ((flags & OCVAR_ORIENT_POSE) && orient_mirrors(orientation)) return refuse(c, who, "OCVAR_ORIENT_POSE with a mirroring orientation: a reflected view has no rigid pose");
    if ((flags & OCVAR_ORIENT_POSE) && !c->have_camera) return refuse(c, who, "OCVAR_ORIENT_POSE without a camera");
    return records_run(c, who, n_frames, stream, [&](int f0, int n, hipStream_t s) {
        launch_orient_records(OrientRecArgs{recs_at(d_markers, f0, records_per_frame), recs_at(d_out, f0, records_per_frame), d_counts + f0,
                                            records_per_frame, src_width, src_height, orientation, flags, c->h_camera}, n, s);
    });
}

extern "C" int ocvar_hip_orient_camera(const OcvarCamera* in, int orientation, OcvarCamera* out) {
    static_assert(sizeof(OcvarCamera) == sizeof(CameraRec), "the same 248 bytes");
    if (!in || !out) return OCVAR_E_ARG;
    return orient_camera(*reinterpret_cast<const CameraRec*>(in), orientation, reinterpret_cast<CameraRec*>(out)) ? OCVAR_OK : OCVAR_E_ARG;
}

extern "C" int ocvar_hip_warp(OcvarHip* c, const uint8_t* d_src, int src_width, int src_height, int src_row_stride, size_t src_frame_stride,
                              uint8_t* d_dst, int dst_width, int dst_height, int dst_row_stride, size_t dst_frame_stride, int n_frames, int format,
                              const double* d_maps, int interpolation, int border, const uint8_t* fill, int flags, int* d_status, void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!d_src || !d_dst || !d_maps) return refuse(c, "warp", "no source frames, no destination frames or no maps");
    constexpr FrameTexts texts = with(TEXTS, FRAMES_FORMAT, "an unknown format, interpolation or border");
    if (!warp_interp_ok(interpolation) || !warp_border_ok(border)) return refuse(c, "warp", texts.why[FRAMES_FORMAT]);
    if (flags & ~WARP_FLAGS) return refuse(c, "warp", "unknown flag bits");
    const int bpp = format_bpp(format);
    if (int rc = pair_check(c, "warp", block_of(d_src, src_width, src_height, bpp, src_row_stride, src_frame_stride, n_frames),
                            block_of(d_dst, dst_width, dst_height, bpp, dst_row_stride, dst_frame_stride, n_frames), ANY_SIZE, texts, "warping"))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    const bool one = (flags & OCVAR_WARP_ONE_MAP) != 0;
    return run_chunks(c, "warp", n_frames, WARP_CHUNK_FRAMES, s, [&](int f0, int n) {
        WarpArgs a{d_src + (size_t)f0 * src_frame_stride, d_dst + (size_t)f0 * dst_frame_stride, src_width, src_height, dst_width, dst_height,
                   (long long)src_row_stride, (long long)src_frame_stride, (long long)dst_row_stride, (long long)dst_frame_stride,
                   one ? d_maps : d_maps + 9 * (size_t)f0, d_status ? d_status + f0 : nullptr, interpolation, border, flags,
                   c->tune[OCVAR_TUNE_WARP_DIRECT] == 1, {0, 0, 0, 0}};
        for (int k = 0; k < 4; k++) a.fill[k] = fill ? fill[k] : 0;
        launch_warp(a, n, format, s);
    });
}

extern "C" int ocvar_hip_warp_records(OcvarHip* c, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int records_per_frame,
                                      const double* d_maps, int flags, OcvarMarker* d_out, void* stream) {
    if (!c) return OCVAR_E_ARG;
    const char* const who = "warp_records";
    if (int rc = records_check(c, who, d_markers && d_counts && d_maps && d_out, n_frames, records_per_frame, "no records, no counts, no maps or no output"))
        return rc;
    if (flags & ~WARP_REC_FLAGS) return refuse(c, who, "unknown flag bits");
    if (flags & OCVAR_WARP_INVERSE_MAP) return refuse(c, who, "OCVAR_WARP_INVERSE_MAP: the records need the forward map");
    if ((flags & OCVAR_WARP_POSE) && !c->have_camera) return refuse(c, who, "OCVAR_WARP_POSE without a camera");
    return records_run(c, who, n_frames, stream, [&](int f0, int n, hipStream_t s) {
        launch_warp_records(WarpRecArgs{recs_at(d_markers, f0, records_per_frame), recs_at(d_out, f0, records_per_frame), d_counts + f0,
                                        records_per_frame, (flags & OCVAR_WARP_ONE_MAP) ? d_maps : d_maps + 9 * (size_t)f0, flags, c->h_camera}, n, s);
    });
}

extern "C" int ocvar_hip_board_plane_maps(OcvarHip* c, const OcvarBoardPose* d_poses, int n_frames, const double* rect, int dst_width,
                                          int dst_height, double* d_maps, void* stream) {
    if (!c) return OCVAR_E_ARG;
    const char* const who = "board_plane_maps";
    if (!d_poses || !rect || !d_maps) return refuse(c, who, "no poses, no rectangle or no maps");
    if (n_frames < 1) return refuse(c, who, "n_frames >= 1");
    if (!any_size_ok(dst_width, dst_height)) return refuse(c, who, TEXTS.why[FRAMES_SIDE]);
    if (!c->have_camera) return refuse(c, who, "no camera set");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    WarpBoardMapArgs a{d_poses, d_maps, n_frames, dst_width, dst_height, {}, {}};
    for (int i = 0; i < 9; i++) a.K[i] = c->h_camera.cameraMatrix[i];
    for (int i = 0; i < 4; i++) a.rect[i] = rect[i];
    launch_warp_board_maps(a, s);
    TRACE_LAUNCH(who, s);
    HIP_TRY(c, hipGetLastError());
    return OCVAR_OK;
}

extern "C" int ocvar_hip_levels_default_params(OcvarLevelsParams* params) {
    if (!params) return OCVAR_E_ARG;
    levels_default_params(params);
    return OCVAR_OK;
}

extern "C" int ocvar_hip_levels(OcvarHip* c, const uint8_t* d_src, int width, int height, int src_row_stride, size_t src_frame_stride, int format,
                                uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride, int n_frames, const OcvarLevelsParams* params,
                                void* stream) {
    if (!c) return OCVAR_E_ARG;
    if (!d_src || !d_dst) return refuse(c, "levels", "no source frames or no destination planes");
    // (the destination is GRAY: one byte per pixel whatever the source's format)
    constexpr FrameTexts texts = with(TEXTS, FRAMES_ROW_STRIDE, "a row stride below the bytes per pixel times width (the destination is GRAY: below width)");
    if (int rc = pair_check(c, "levels", block_of(d_src, width, height, format_bpp(format), src_row_stride, src_frame_stride, n_frames),
                            block_of(d_dst, width, height, 1, dst_row_stride, dst_frame_stride, n_frames), ANY_SIZE, texts, "levels", true, "source and destination"))
        return rc;
    OcvarLevelsParams p;
    levels_default_params(&p);
    if (params) p = *params;
    static const char* const why[] = {"", "tiles_x and tiles_y 1 .. 16, at most 64 tiles, no more tiles than pixels along an axis",
                                      "low_ppm and high_ppm 0 .. 500000", "max_gain_q8 256 .. 65280"};
    if (const int bad = levels_params_bad(p, width, height)) return refuse(c, "levels", why[bad]);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    const bool fresh = c->levels_ws.bytes == 0;
    HIP_TRY(c, c->levels_ws.reserve((size_t)LEVELS_WS_BYTES));
    HIP_TRY(c, c->levels_fence.enter(s));
    // the histograms start as zeros; every round's LUT kernel leaves them so
    if (fresh) HIP_TRY(c, hipMemsetAsync(c->levels_ws, 0, (size_t)LEVELS_WS_LUT_OFFSET, s));
    const int rc = run_chunks(c, "levels", n_frames, LEVELS_WS_FRAMES, s, [&](int f0, int n) {     // the rounds share the workspace in stream order
        const LevelsArgs a{d_src + (size_t)f0 * src_frame_stride, d_dst + (size_t)f0 * dst_frame_stride, width, height,
                           (long long)src_row_stride, (long long)src_frame_stride, (long long)dst_row_stride, (long long)dst_frame_stride, p,
                           reinterpret_cast<unsigned*>(c->levels_ws.p), c->levels_ws.p + LEVELS_WS_LUT_OFFSET};
        launch_levels(a, n, format, s);
    });
    if (rc) return rc;
    HIP_TRY(c, c->levels_fence.leave(s));
    return OCVAR_OK;
}

extern "C" int ocvar_hip_bayer_default_params(OcvarBayerParams* p) {
    if (!p) return OCVAR_E_ARG;
    bayer_default_params(p);
    return OCVAR_OK;
}

extern "C" int ocvar_hip_bayer_pattern_at(int pattern, int x0, int y0) { return bayer_pattern_at(pattern, x0, y0); }

extern "C" int ocvar_hip_bayer_to_frames(OcvarHip* c, const void* d_src, int src_row_stride, size_t src_frame_stride, uint8_t* d_dst,
                                         int dst_row_stride, size_t dst_frame_stride, int width, int height, int n_frames, int format,
                                         const OcvarBayerParams* params, void* stream) {
    static_assert(sizeof(OcvarBayerParams) == 24, "the 24 bytes of the header");
    if (!c) return OCVAR_E_ARG;
    const char* const who = "bayer_to_frames";
    if (!d_src || !d_dst) return refuse(c, who, "no source mosaics or no destination frames");
    OcvarBayerParams p;
    bayer_default_params(&p);
    if (params) p = *params;
    constexpr const char* UNKNOWN = "an unknown pattern or format";
    static const char* const why[] = {"", UNKNOWN, "bits 8 .. 16", "black 0 .. 2^bits - 1", "gains 0 .. 16383"};
    if (const int bad = bayer_params_bad(p)) return refuse(c, who, why[bad]);
    constexpr FrameTexts texts = with(with(with(TEXTS, FRAMES_FORMAT, UNKNOWN), FRAMES_SIDE, "sides of 2 .. 32767 pixels"), FRAMES_ROW_STRIDE,
                                      "a row stride below the row's bytes (the source: the sample's bytes times width)");
    if (width < 2 || height < 2) return refuse(c, who, texts.why[FRAMES_SIDE]);
    const int sb = bayer_sample_bytes(p.bits);
    if (sb == 2 && (((uintptr_t)d_src | (uintptr_t)src_row_stride | (uintptr_t)src_frame_stride) & 1))
        return refuse(c, who, "a 16-bit source at an odd address or with an odd stride");
    const uint8_t* src = static_cast<const uint8_t*>(d_src);
    // (the destination first: of the two blocks it alone can have an unknown format)
    if (int rc = pair_check(c, who, block_of(d_dst, width, height, format_bpp(format), dst_row_stride, dst_frame_stride, n_frames),
                            block_of(src, width, height, sb, src_row_stride, src_frame_stride, n_frames), ANY_SIZE, texts, "demosaic", true,
                            "source and destination"))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = stream_or_own(c, stream);
    const int pairs = c->tune[OCVAR_TUNE_BAYER_PAIRS] > 0 ? std::min(c->tune[OCVAR_TUNE_BAYER_PAIRS], BAYER_MAX_PAIRS) : BAYER_PAIRS;
    return run_chunks(c, who, n_frames, BAYER_CHUNK_FRAMES, s, [&](int f0, int n) {
        const BayerArgs a{src + (size_t)f0 * src_frame_stride, d_dst + (size_t)f0 * dst_frame_stride, (long long)src_row_stride,
                          (long long)src_frame_stride, (long long)dst_row_stride, (long long)dst_frame_stride, width, height, format, p, pairs};
        launch_bayer(a, n, s);
    });
}

// a parameter of ocvar_hip_flow_records that must be a finite number >= 0
static bool flow_number_ok(float v) { return v >= 0.0f && v <= 3.0e38f; }

extern "C" int ocvar_hip_flow_records(OcvarHip* c, const uint8_t* d_prev_frames, int prev_row_stride, size_t prev_frame_stride,
                                      const uint8_t* d_next_frames, int next_row_stride, size_t next_frame_stride, int width, int height,
                                      int n_frames, int format, const OcvarMarker* d_markers, const int* d_counts, int records_per_frame,
                                      const OcvarFlowParams* params, OcvarMarker* d_out, int* d_status, float* d_err, void* stream) {
    if (!c) return OCVAR_E_ARG;
    const char* const who = "flow_records";
    const OcvarFlowParams p = params ? *params : OcvarFlowParams{10, 3, 30, 0, 0.03f, 1e-3f, 0.0f, 0.0f};
    if (int rc = records_check(c, who, d_prev_frames && d_next_frames && d_markers && d_counts && d_out, n_frames, records_per_frame,
                               "no frames, no records, no counts or no output"))
        return rc;
    if (p.half_win < 1 || p.half_win > OCVAR_MAX_FLOW_HALF_WIN || p.levels < 0 || p.levels > OCVAR_MAX_FLOW_LEVELS || p.max_iter < 1 || p.max_iter > 100)
        return refuse(c, who, "half_win 1 .. " + std::to_string(OCVAR_MAX_FLOW_HALF_WIN) + ", levels 0 .. " + std::to_string(OCVAR_MAX_FLOW_LEVELS) +
                                  ", max_iter 1 .. 100");
    if (!flow_number_ok(p.eps) || !flow_number_ok(p.min_eig) || !flow_number_ok(p.max_err) || !flow_number_ok(p.fb_max))
        return refuse(c, who, "eps, min_eig, max_err and fb_max are finite numbers >= 0");
    if (p.flags & ~FLOW_FLAGS) return refuse(c, who, "unknown flag bits");
    const int side = 2 * p.half_win + 3, bpp = format_bpp(format);
    constexpr const char* FORMAT_OR_STRIDE = "an unknown format or a row stride below the format's bytes per pixel times width";
    constexpr FrameTexts texts = with(with(with(TEXTS, FRAMES_SIDE, "frames of 2 half_win + 3 pixels each way .. the context's size"), FRAMES_FORMAT,
                                           FORMAT_OR_STRIDE), FRAMES_ROW_STRIDE, FORMAT_OR_STRIDE);
    if (width < side || height < side) return refuse(c, who, texts.why[FRAMES_SIDE]);
    if (int rc = block_check(c, who, block_of(d_prev_frames, width, height, bpp, prev_row_stride, prev_frame_stride, n_frames), context_size(c), texts, false)) return rc;
    if (int rc = block_check(c, who, block_of(d_next_frames, width, height, bpp, next_row_stride, next_frame_stride, n_frames), context_size(c), texts, false)) return rc;
    if (int rc = frame_span_check(c, width, height, prev_row_stride, format)) return rc;
    if (int rc = frame_span_check(c, width, height, next_row_stride, format)) return rc;
    if ((p.flags & OCVAR_FLOW_POSE) && !c->have_camera) return refuse(c, who, "OCVAR_FLOW_POSE without a camera");
    HIP_TRY(c, hipSetDevice(c->device));
    const int chunk = std::min(c->ws.max_batch, 32);
    const size_t slot = (size_t)flow_geom(c->ws.max_w, c->ws.max_h, 1, 0).bytes;
    HIP_TRY(c, c->flow_ws.reserve(2 * (size_t)chunk * slot));
    const hipStream_t s = stream_or_own(c, stream);
    HIP_TRY(c, c->flow_fence.enter(s));
    const FlowGeom g = flow_geom(width, height, p.half_win, p.levels);
    uint8_t* pyr_a = c->flow_ws;
    uint8_t* pyr_b = pyr_a + (size_t)chunk * slot;
    const int rc = run_chunks(c, "flow_track", n_frames, chunk, s, [&](int f0, int n) {
        launch_flow_pyramids(FlowPyrArgs{d_prev_frames + (size_t)f0 * prev_frame_stride, (long long)prev_row_stride, (long long)prev_frame_stride,
                                         pyr_a, (long long)slot, g}, n, format, s);
        launch_flow_pyramids(FlowPyrArgs{d_next_frames + (size_t)f0 * next_frame_stride, (long long)next_row_stride, (long long)next_frame_stride,
                                         pyr_b, (long long)slot, g}, n, format, s);
        TRACE_LAUNCH("flow_pyramids", s);
        const size_t r0 = (size_t)f0 * records_per_frame;
        launch_flow_track(FlowTrackArgs{pyr_a, pyr_b, (long long)slot, g, flow_args_make(p), c->h_camera, recs_at(d_markers, f0, records_per_frame),
                                        d_counts + f0, recs_at(d_out, f0, records_per_frame), d_status ? d_status + r0 : nullptr,
                                        d_err ? d_err + 4 * r0 : nullptr, records_per_frame, n}, s);
    });
    if (rc) return rc;
    HIP_TRY(c, c->flow_fence.leave(s));
    return OCVAR_OK;
}
