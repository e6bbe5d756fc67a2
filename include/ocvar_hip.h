/*
 * ocvar_hip.h -- thin C ABI of the MI355X (gfx950) AR-marker detection path.
 *
 * This is the drop-in boundary for the reference's one hot path, cvarArMultRegistration
 * (/root/reference/include/opencvar/opencvar.h:259-260, /root/reference/src/opencvar.cpp:619-807) and the
 * functions under it.  Plain pointers and sizes only; no C++ or torch types.  The host-side C++ mirror of
 * the reference API (include/opencvar/opencvar.h in this repo) is a thin caller of these entry points.
 *
 * Which reference interface each entry point stands in for:
 *   ocvar_hip_set_templates  <- the vector<CvarTemplate> argument (opencvar.h:65-70, filled by
 *                               cvarLoadTemplateTag/cvarLoadTag, opencvar.cpp:284-321)
 *   ocvar_hip_set_camera     <- the CvarCamera* argument (opencvar.h:54-60; cvarReadCamera/cvarCameraScale,
 *                               opencvar.cpp:39-104)
 *   ocvar_hip_detect_*       <- cvarArMultRegistration for a batch of independent frames (stateless when
 *                               prev == NULL; with prev it replays the tracking stage, opencvar.cpp:635-668)
 *   ocvar_hip_find_squares   <- cvarFindSquares + cvarGetAllSquares (opencvar.h:131,240; opencvar.cpp:156-223,564-590)
 *   ocvar_hip_debug_*        <- no reference counterpart: parity hooks (binary image, pre-dedupe candidates)
 *
 * All functions return 0 on success and a negative OCVAR_E_* code on failure; none throws.  There is no
 * CPU fallback: without a gfx950 device ocvar_hip_create fails.
 */
#ifndef OCVAR_HIP_H
#define OCVAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Layout-identical to the reference's PODs (opencvar.h:54-82); sizes 248 / 48 / 184 bytes. */
typedef struct { int width, height; double cameraMatrix[9]; double distCoeffs[5]; double glProjection[16]; } OcvarCamera;
typedef struct { int width, height; double scale; long long code[4]; } OcvarTemplate;
typedef struct {
    double glMatrix[16]; int templateId; int markerId; double score; float square[8]; double aspectRatio;
} OcvarMarker;

/* Pre-dedupe candidate (one per frame-pass quad with a crop-pass quad, per template); SURVEY.md 8(d). */
typedef struct {
    int markerId, templateId, orient, valid;
    long long bit;
    float square[8];
    float patPoint[8];
} OcvarCandidate;

typedef struct OcvarHip OcvarHip;

enum {
    OCVAR_OK = 0,
    OCVAR_E_NO_DEVICE = -1,   /* no HIP device / not gfx950 */
    OCVAR_E_ARG = -2,
    OCVAR_E_HIP = -3,         /* a HIP runtime call failed; see ocvar_hip_last_error */
    OCVAR_E_CAPACITY = -4     /* a device work list overflowed (frame too cluttered for the configured limits) */
};

/* Templates per context: up to OCVAR_MAX_TEMPLATES, each of at most 64 code cells (width x height), in at most
 * OCVAR_MAX_TEMPLATE_SIZES distinct (width, height) code sizes; ocvar_hip_set_templates returns OCVAR_E_ARG beyond either.
 * Identical templates and rotationally symmetric codes are allowed, as in the reference. */
enum { OCVAR_MAX_TEMPLATES = 4096, OCVAR_MAX_TEMPLATE_SIZES = 16, OCVAR_MAX_QUADS = 256, OCVAR_MAX_MARKERS = 64,
       OCVAR_MAX_QUADS_EX = 1792 /* most squares per frame a context can be created for (ocvar_hip_create_ex) */,
       OCVAR_MAX_QUADS_DENSE = 16384, OCVAR_MAX_MARKERS_DENSE = 4096 /* limits of ocvar_hip_create_dense */ };

/* Creates a context on `device` with workspace for batches of up to max_batch frames of up to
 * max_width x max_height pixels. */
int ocvar_hip_create(OcvarHip** ctx, int device, int max_width, int max_height, int max_batch);
/* Same with room for max_quads (1 .. OCVAR_MAX_QUADS_EX) frame-pass squares per frame instead of OCVAR_MAX_QUADS: the
 * reference's square list is unbounded (opencvar.cpp:187-214); a caller that gets OCVAR_E_CAPACITY with flag 4 (squares)
 * repeats the frame on such a context (the host mirror of cvarArMultRegistration / cvarFindSquares does). */
int ocvar_hip_create_ex(OcvarHip** ctx, int device, int max_width, int max_height, int max_batch, int max_quads);
/* A dense context: room for max_quads (1 .. OCVAR_MAX_QUADS_DENSE) frame-pass squares and max_markers (1 ..
 * OCVAR_MAX_MARKERS_DENSE) markers per frame, tracked plus new -- the reference bounds neither (opencvar.cpp:187-214, 619-807).
 * OCVAR_E_ARG outside those ranges, checked before any device call.  The per-frame tail runs in scalable kernels (a sort of
 * the squares in place of an O(n^2) rank, a sparse replay of the tracking loop, global workspace in place of LDS); results are
 * those of any other context.  The marker stride M of every [n][M] array below is max_markers (ocvar_hip_max_markers).
 * Footprint per frame of max_batch, with W x H = max_width x max_height, Q = max_quads, M = max_markers: device ~480 Q bytes
 * (square lists, crop records, the dense tail's sort / grid / replay arrays) + 380 M bytes (prev, reserve, markers, pose jobs)
 * + a crop pool of 4 (W + 16) (H + 8) bytes (four times a default context's: crops of neighbouring squares overlap) + W H / 128
 * bytes (tracking grid) + the per-square decode tables of ocvar_hip_set_templates (8 bytes per template size class and 4 per
 * match of the library, per square); pinned host 368 M bytes (result and `prev` staging).  At 4K with Q = 16384, M = 4096:
 * ~43 MB of device memory and 1.5 MB pinned per frame, besides the frame planes every context holds. */
int ocvar_hip_create_dense(OcvarHip** ctx, int device, int max_width, int max_height, int max_batch, int max_quads, int max_markers);
/* The context's marker stride M: max_markers of ocvar_hip_create_dense, OCVAR_MAX_MARKERS on a context made by
 * ocvar_hip_create / ocvar_hip_create_ex.  OCVAR_E_ARG for NULL. */
int ocvar_hip_max_markers(const OcvarHip* ctx);
void ocvar_hip_destroy(OcvarHip* ctx);
const char* ocvar_hip_last_error(const OcvarHip* ctx);
/* Flag word of the last call that failed with OCVAR_E_CAPACITY: 1 start lists, 2 point pool, 4 squares / candidates per
 * frame, 8 trace overrun, 16 crops, 32 crop tiles, 64 work-queue runaway, 128 markers per frame (more than the context's
 * M = ocvar_hip_max_markers).  0 after a good call. */
int ocvar_hip_capacity_flags(const OcvarHip* ctx);

/* Several contexts in flight on one GPU overlap the latency-bound border followers of one batch with the streaming binarise
 * kernels of another -- but left alone they drift: a quarter of the time none of them is in a binarise kernel and a sixth of
 * the time three are (rocprofv3 trace of bench.py).  A gate shared by the contexts lets at most `width`
 * binarise kernels run at once (stream-ordered: the n-th binarise launch waits for the (n - width)-th to finish; nothing
 * blocks on the host), so that more contexts can be kept in flight to always have one ready.
 *
 * The gate is also the scheduler of its contexts' batches.  Streams that share a hardware queue run one after the other, and
 * a process has few queues (GPU_MAX_HW_QUEUES, four by default; the library reads the variable and never sets it).  So the
 * gate owns one stream per queue -- a "lane"; at most 8, created together so that they land on distinct queues -- and a
 * batch enqueued with stream == NULL on a context of the gate runs on the lane with the least outstanding work at that moment
 * (ties: the lane whose newest batch is oldest), not on the context's own stream.  More contexts than lanes is the intended
 * use: the batch queued behind another keeps its lane busy while the host collects and re-enqueues.  Create the gate before
 * the contexts (and before other streams) where queues are scarce: streams made earlier have taken their queues by then.
 * A context without a gate, and every call that names a stream, are untouched by this.
 * No counterpart in the reference (it processes one frame per call). */
typedef struct OcvarGate OcvarGate;
int ocvar_hip_gate_create(OcvarGate** gate, int device, int width);
/* The same with the number of lanes chosen by the caller (1..8; 0: from the queue count as above) -- for experiments and
 * tests; results do not depend on it. */
int ocvar_hip_gate_create_lanes(OcvarGate** gate, int device, int width, int lanes);
int ocvar_hip_gate_lanes(const OcvarGate* gate);
/* Waits for the work on the gate's lanes.  Contexts still attached are detached (they go on without a gate; a batch one of
 * them has in flight is complete by then and is collected as usual). */
void ocvar_hip_gate_destroy(OcvarGate* gate);
/* gate may be NULL (no gate: the default).  The gate keeps the order of its gated launches on the host without locks, so the
 * contexts that share one are enqueued from one host thread; they may be collected and destroyed from other threads (the lanes'
 * bookkeeping is locked).  Changing the gate of a context whose batch runs on a lane of the old gate waits for that batch. */
int ocvar_hip_set_gate(OcvarHip* ctx, OcvarGate* gate);

int ocvar_hip_set_templates(OcvarHip* ctx, const OcvarTemplate* templates, int n);
int ocvar_hip_set_camera(OcvarHip* ctx, const OcvarCamera* camera);

/* Input formats: what the frames handed to the detection entry points hold (d_bgr / h_bgr below keep their names).  8-bit
 * interleaved pixels of 3, 3, 4, 4 and 1 bytes; row_stride must be at least that many bytes times width (else OCVAR_E_ARG).
 * The rows of one frame must lie within 2^31 - 1 bytes of its first byte, which is as far as the frame kernel addresses: with
 * bpp the bytes per pixel,
 *     ((height & ~1) - 1) * row_stride + bpp * (width & ~1) <= 2147483647
 * else OCVAR_E_ARG with a text in ocvar_hip_last_error, before any device call and with the frames untouched -- from every
 * entry point that takes frames (detect_device, enqueue, enqueue_tracked, the pipe calls, detect_host on the caller's host
 * strides, find_squares on its 3 * width expansion).  It binds views into a large surface (a big row_stride) and frames
 * above about 26755 x 26755 BGR / 23170 x 23170 BGRA; frame_stride, and so the batch, are not limited by it.
 * Parity: a frame in format F gives exactly what the reference gives on the BGR frame with the same colours --
 *   OCVAR_FMT_GRAY  B = G = R = g (the reference's BGR2GRAY of such a pixel is g)
 *   OCVAR_FMT_RGB   the channels reversed
 *   OCVAR_FMT_BGRA / OCVAR_FMT_RGBA  the fourth byte is ignored
 * grey_in_place writes the grey value into bytes 0..2 of every pixel (a four-channel pixel's byte 3 is left as it is); in
 * OCVAR_FMT_GRAY it does nothing (no kernel, and ocvar_hip_detect_host copies nothing back).
 * YUV sources (NV12, I420): OCVAR_FMT_GRAY on the luma plane -- row_stride = the plane's pitch, frame_stride = the whole
 * YUV frame's size (pitch * height * 3 / 2 for NV12 and I420 with a common pitch); the chroma bytes are never read.  The result
 * is the reference on the luma image.  For the reference on the colour conversion of the YUV frame, and for everything that needs
 * colour (overlays, patches, undistortion), convert on the device first: ocvar_hip_yuv_to_frames below. */
enum { OCVAR_FMT_BGR = 0, OCVAR_FMT_RGB = 1, OCVAR_FMT_BGRA = 2, OCVAR_FMT_RGBA = 3, OCVAR_FMT_GRAY = 4 };
/* Context state like the result limit and the camera: read when a batch is enqueued, by every entry point that takes frames
 * (detect_device, enqueue, enqueue_tracked, detect_host).  Default OCVAR_FMT_BGR.  OCVAR_E_ARG for an unknown format, or
 * while the context has a batch that has not been collected.  ocvar_hip_find_squares takes a grey image whatever the
 * format. */
int ocvar_hip_set_input_format(OcvarHip* ctx, int format);

/* Sub-pixel corner refinement (off by default): every marker record a batch writes, tracked or new, gets its four square
 * corners refined on that frame's grey image with the equations of OpenCV's cornerSubPix (opencv-ar_amd/csrc/refine_core.h),
 * and its glMatrix is solved from the refined corners.  Frame quads, crop quads, candidates, and which markers come out with
 * which ids, templates and scores do not change.  With tracking, the refined squares a caller hands back as `prev` are what
 * the next frame's 20-px rule compares.
 *   half_win  0 (off) .. OCVAR_MAX_REFINE_HALF_WIN: the window is (2 half_win + 1)^2 px around the corner
 *   max_iter  1 .. 100 steps per corner
 *   eps       >= 0 px: a corner stops once a step moves it by at most eps
 * ArUco's typical setting is 5 / 30 / 0.1.  OCVAR_E_ARG outside those ranges, before any device call.  Applies from the next
 * enqueue (a batch in flight keeps the setting it was enqueued with). */
enum { OCVAR_MAX_REFINE_HALF_WIN = 15 };
int ocvar_hip_set_corner_refine(OcvarHip* ctx, int half_win, int max_iter, float eps);

/* Planar marker board (off by default): one rigid pose per frame from every board marker the frame's records hold -- ArUco's
 * estimatePoseBoard, ARToolKit's multi-marker set (opencv-ar_amd/csrc/board_core.h).  An entry names a template and the board
 * plane (z = 0) coordinates of the marker's corners 0..3.  Corner c is the point the code[0] readout puts at corner c of the
 * readout's destination rectangle (0,0), (W-1,0), (W-1,H-1), (0,H-1); since templates are loaded flipped vertically, corners 0..3
 * are the template image's bottom-left, bottom-right, top-right and top-left corners (and corners 0..3 of OcvarSynthMarker.corner
 * for a marker ocvar_synth_* draws).
 * Per frame the board takes, of every entry, the first record in output order with score > 0 and the entry's template, reads
 * that record's code again on the frame's grey image at the record's square (refined when corner refinement is on) to find which
 * record corner is which board corner (no match: the marker is not used), seeds from the (up to) 4 used markers of largest image
 * area and refines with Levenberg-Marquardt over all used corners, with the context's camera (intrinsics and distortion).
 * Entries whose template is absent from the current library, or is not square (width != height), never match.
 * ocvar_hip_set_board: n = 0 turns the board off; OCVAR_E_ARG, before any device call, for n outside 0..OCVAR_MAX_BOARD_MARKERS,
 * a template id outside 0..OCVAR_MAX_TEMPLATES-1 or repeated, a coordinate that is not finite, corners that are not a convex quad
 * of non-zero area, or while the context has a batch that has not been collected.  Applies from the next enqueue.  With no board
 * nothing changes: no launch, no copy.  Markers and counts never depend on the board. */
enum { OCVAR_MAX_BOARD_MARKERS = 256 };
/* one marker of a planar board: its template and the board-plane (z = 0) coordinates of its 4 corners; 72 bytes */
typedef struct { int templateId; int pad; double corner[8]; } OcvarBoardMarker;
typedef struct {
    double glMatrix[16];     /* board frame -> GL modelview, the convention of a marker record (cvarGlMatrix) */
    double rvec[3], tvec[3]; /* OpenCV convention: X_cam = R(rvec) X_board + tvec, in board units */
    double rms;              /* RMS reprojection error over the corners used, px */
    int n_markers;           /* board markers used in this frame */
    int status;              /* 1 solved, 0 no board marker found, -1 not solvable (degenerate seeds / non-finite) */
} OcvarBoardPose;            /* 192 bytes */
int ocvar_hip_set_board(OcvarHip* ctx, const OcvarBoardMarker* markers, int n);
/* The poses [n_frames] of the last collected batch (all frames of an ocvar_hip_detect_host call); OCVAR_E_ARG when that batch had
 * no board, or for n_frames outside 1 .. its frame count. */
int ocvar_hip_board_poses(OcvarHip* ctx, OcvarBoardPose* poses, int n_frames);
/* After ocvar_hip_enqueue (like ocvar_hip_results_to_device): stream-ordered copy of the batch's poses into d_poses [n_frames]
 * in device memory.  OCVAR_E_ARG when nothing is enqueued or the batch has no board. */
int ocvar_hip_board_poses_to_device(OcvarHip* ctx, OcvarBoardPose* d_poses, void* stream);

/* Overlays (none by default): an RGBA image per template, warped into the quad of every marker record and blended into frames
 * that stay in device memory -- what the reference's caller does with its records (samples/ARTest.cpp draws on every marker),
 * without GL.  The definition, bit for bit, is opencv-ar_amd/csrc/overlay_core.h: the map perspective_from_quad(record.square)
 * from frame pixels to texels in float32, texel coordinates in 1/32, plain bilinear sampling (no mipmaps, no anti-aliased
 * edges), straight alpha, out = (c a + d (255 - a) + 127) / 255 per colour channel; alpha 0 leaves the pixel untouched; byte 3
 * of a four-channel pixel is never written; OCVAR_FMT_GRAY takes the library's grey of the colour.  Of a frame's records the
 * first min(count, stride) are drawn in output order, later over earlier, each with score > 0 whose template has an overlay
 * (or the default overlay) and whose four corners are finite and a strictly convex quad.
 * Which way up: the overlay's top-left, top-right, bottom-right and bottom-left texels land on record corners 0, 1, 2, 3.  For a
 * marker decoded at orient 1, 2 or 4 those are the template image's bottom-left, bottom-right, top-right and top-left corners
 * however the marker is turned in the frame (templates are loaded flipped vertically, see ocvar_hip_set_board below): the overlay
 * lies on the marker as its printed pattern does, the image's top row along the template image's bottom row.  A marker decoded
 * at orient 3 (turned by 180 degrees against orient 1) keeps its corners as found, as in the reference (opencvar.cpp:753-760
 * rotates for orient 2 and 4 only): its record, its glMatrix and its overlay are turned by 180 degrees on it.
 *
 * ocvar_hip_set_overlay: h_rgba is a host image of width x height texels (2 .. OCVAR_MAX_OVERLAY_SIDE each), 4 bytes R G B A per
 * texel, rows row_stride >= 4 width bytes apart; it is copied to device memory.  template_id 0 .. OCVAR_MAX_TEMPLATES-1, or -1:
 * the default overlay, used for every template without one of its own.  h_rgba == NULL removes that overlay.  At most
 * OCVAR_MAX_OVERLAYS per context, the default included.  OCVAR_E_ARG, before any device call, for a size outside the range, a
 * row_stride below 4 width, a bad id, one overlay more than OCVAR_MAX_OVERLAYS, or while the context has a batch that has not
 * been collected.  The first overlay allocates the drawing workspace (64 bytes per marker record of max_batch frames); a
 * context without overlays allocates and launches nothing.  Markers, counts and board poses never depend on overlays. */
enum { OCVAR_MAX_OVERLAYS = 64, OCVAR_MAX_OVERLAY_SIDE = 1024 };
int ocvar_hip_set_overlay(OcvarHip* ctx, int template_id, const uint8_t* h_rgba, int width, int height, int row_stride);
/* After ocvar_hip_enqueue and before ocvar_hip_collect (like ocvar_hip_results_to_device, with the same promises about streams,
 * lanes and collect on a context of a gate): draws the enqueued batch's own records onto d_frames -- the frames that were
 * detected (after grey_in_place, if that was asked for) or any other buffer of the batch's frame count and size -- in `format`
 * (OCVAR_FMT_*; it need not be the input format).  Stream-ordered behind the batch; does not wait.  OCVAR_E_ARG when nothing is
 * enqueued, no overlay is set, width or height differ from the batch's, the format is unknown or row_stride is below the
 * format's bytes per pixel times width. */
int ocvar_hip_render(OcvarHip* ctx, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int format,
                     void* stream);
/* The same on records the caller supplies in device memory, d_markers [n_frames][records_per_frame] and d_counts [n_frames]
 * (1 <= records_per_frame <= M = ocvar_hip_max_markers(ctx); a count above records_per_frame is read as records_per_frame) --
 * gathered, filtered or smoothed records, say.  Needs no batch; frames of up to the context's max_width x max_height; any
 * n_frames >= 1 (more than max_batch go through the workspace in chunks, in stream order).  stream NULL: the context's own
 * stream.  Does not wait.  OCVAR_E_ARG for a size, stride or format as above or when no overlay is set. */
int ocvar_hip_render_records(OcvarHip* ctx, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride,
                             int n_frames, int format, const OcvarMarker* d_markers, const int* d_counts, int records_per_frame,
                             void* stream);

/* Annotation (opt-in): outlines, a corner-0 dot, pose axes, a cube and the template id of every marker record, stroked straight
 * into frames that stay in device memory -- what a caller draws first when setting up a camera or a board (ArUco's
 * drawDetectedMarkers / drawFrameAxes; the reference's sample draws a cube on every square).  The definition, bit for bit, is
 * opencv-ar_amd/csrc/annotate_core.h; it is the library's own stroke rule (parity with OpenCV's line rasteriser is neither claimed
 * nor tested).  In short: a stroke is the set of pixels whose centre lies within thickness / 2 of its segment (round ends; a
 * zero-length segment is a disc), end points rounded once to 1/16 px and clamped to +-OCVAR_ANNO_MAX_COORD px.  Of one record, in
 * this order: the four edges of `square`, a dot of diameter 2 thickness + 1 on corner 0, the twelve edges of a cube on the marker
 * rectangle (+-aspectRatio, +-1, 0) with its top at z = cube_height, the axes X (red), Y (green), Z (blue) of axis_length from the
 * model origin, and templateId in decimal in a 5 x 7 bitmap font, axis-aligned and centred on the mean of the corners.  (R, t) of
 * cube and axes is the inverse of glMatrix's construction; their end points are projected with the context's camera as it is at
 * the call (by value), distortion included, and joined by straight strokes; an end point at camera z <= 0 or with a projection
 * that is not finite drops its segment.  A pixel takes the colour of the last primitive of the record that covers it and is
 * blended once, by the overlay's rule (straight alpha, alpha 0 leaves the pixel untouched, byte 3 of a four-channel pixel is never
 * written, OCVAR_FMT_GRAY takes the library's grey of the colour): joints and crossings of half-transparent strokes do not darken
 * twice.  Records composite in output order, k = 0 .. min(count, stride) - 1, later over earlier.  A record draws when all eight
 * corner coordinates are finite and score > 0; with OCVAR_ANNO_UNMATCHED a record with score <= 0 draws its outline (in the
 * `unmatched` colour) and its corner-0 dot, where those are asked for.  Cube and axes also need a finite glMatrix.  There is no
 * convexity requirement.
 *
 * The style is passed by value with every call; the context keeps none.  ocvar_hip_annotate_default_style (host only: no context,
 * no device call) fills: OUTLINE | CORNER0 | LABEL, thickness 2, axis_length 1, cube_height 1, label_scale 0 (automatic: the
 * largest s in 1 .. 8 with 24 s <= the quad's shortest edge, else 1), outline green, unmatched grey, corner 0 red, cube cyan, label
 * yellow, all opaque.  With OCVAR_ANNO_COLOR_BY_TEMPLATE the outline of a matched record takes colour templateId mod 12 of a fixed
 * palette (annotate_core.h) with the outline's alpha.
 *
 * ocvar_hip_annotate: after ocvar_hip_enqueue and before ocvar_hip_collect, on the enqueued batch's own records, with the same
 * promises about streams, gates, lanes and collect as ocvar_hip_render.  ocvar_hip_render and ocvar_hip_annotate may both be
 * called on one batch: they are stream-ordered in call order (on one stream; a caller who names two streams orders them).
 * ocvar_hip_annotate_records: on records the caller supplies in device memory, as ocvar_hip_render_records: no batch, frames of up
 * to the context's size, any n_frames >= 1 (more than max_batch go through the workspace in chunks, in stream order), stream
 * NULL: the context's own stream.  Neither waits.  The first call allocates the workspace (OCVAR_ANNO_RECORD_BYTES per marker
 * record slot of max_batch frames); a context that never annotates allocates and launches nothing.  Markers, counts and board
 * poses never depend on these calls.  OCVAR_E_ARG, before any device call and with the frames untouched, for a size, stride or
 * format as ocvar_hip_render / ocvar_hip_render_records refuse them, a NULL style, thickness outside 1 .. 16, label_scale outside
 * 0 .. 8, an axis_length or cube_height that is negative or not finite, unknown flag bits, none of OUTLINE, CORNER0, AXES, CUBE
 * and LABEL set, and AXES or CUBE while the context has no camera. */
enum { OCVAR_ANNO_OUTLINE = 1, OCVAR_ANNO_CORNER0 = 2, OCVAR_ANNO_AXES = 4, OCVAR_ANNO_CUBE = 8, OCVAR_ANNO_LABEL = 16,
       OCVAR_ANNO_UNMATCHED = 32, OCVAR_ANNO_COLOR_BY_TEMPLATE = 64,
       OCVAR_ANNO_MAX_THICKNESS = 16, OCVAR_ANNO_MAX_LABEL_SCALE = 8, OCVAR_ANNO_MAX_COORD = 1048576, OCVAR_ANNO_RECORD_BYTES = 696 };
typedef struct {
    int flags;                       /* OCVAR_ANNO_* */
    int thickness;                   /* stroke width in pixels, 1 .. 16 */
    int label_scale;                 /* glyph cell in pixels, 1 .. 8; 0: automatic */
    int reserved;                    /* 0 */
    double axis_length, cube_height; /* in the marker model's units: the marker is (+-aspectRatio, +-1, 0) */
    uint8_t outline[4], unmatched[4], corner0[4], cube[4], label[4];   /* straight-alpha R G B A */
    uint8_t reserved2[4];            /* 0 */
} OcvarAnnotateStyle;   /* 56 bytes */
int ocvar_hip_annotate_default_style(OcvarAnnotateStyle* style);   /* host only, no context, no device call */
int ocvar_hip_annotate(OcvarHip* ctx, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int format,
                       const OcvarAnnotateStyle* style, void* stream);
int ocvar_hip_annotate_records(OcvarHip* ctx, uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride,
                               int n_frames, int format, const OcvarMarker* d_markers, const int* d_counts, int records_per_frame,
                               const OcvarAnnotateStyle* style, void* stream);

/* Patches: the upright, perspective-free image of every marker record, cut out of frames that stay in device memory -- the
 * reference's cvarInvertPerspective(frame, patch, record.square, cvarSquare(patch_w, patch_h, 0)) (opencvar.cpp:510-516), one
 * dense block for a whole batch.  The definition, bit for bit, is opencv-ar_amd/csrc/patch_core.h: the map
 * perspective_from_quad(record.square, patch_w, patch_h) in float32, inverted in double, cvWarpPerspective's 1/32-px bilinear
 * sampling with a constant 0 outside the frame.  Record corners 0, 1, 2, 3 land on patch pixels (0,0), (patch_w-1,0),
 * (patch_w-1,patch_h-1), (0,patch_h-1).  Every byte of a pixel is warped alike: a patch has the bytes per pixel of `format`
 * (1, 3 or 4) in the frame's memory order, byte 3 of a four-channel pixel included.
 *   d_patches  [n_frames][records_per_frame][patch_h][patch_w][bpp] bytes, contiguous, at any address
 *   d_status   [n_frames][records_per_frame] ints, every entry written; may be NULL
 * A slot is written (status 1) when its index is below min(count, records_per_frame), all eight coordinates of the square are
 * finite and at most 1e6 (OCVAR_PATCH_MAX_COORD) in magnitude, the quad has a map (four corners in a line have none) and, with
 * OCVAR_PATCH_MATCHED_ONLY, score > 0.  Every other slot gets status 0 and none of its patch bytes is touched.  A written patch
 * wholly outside the frame is all zeros.  Quads that are not convex give whatever the formulas give.
 * OCVAR_PATCH_FLIP_ROWS stores patch row r at row patch_h-1-r and changes nothing else: templates are loaded flipped vertically
 * (see ocvar_hip_set_board), so with this flag a marker's patch reads like its template's image file.
 *
 * ocvar_hip_patches: after ocvar_hip_enqueue and before ocvar_hip_collect (like ocvar_hip_render, with the same promises about
 * streams, lanes and collect on a context of a gate), on the enqueued batch's own records, the first records_per_frame (1 .. M =
 * ocvar_hip_max_markers(ctx)) of every frame.  d_frames: the frames that were detected (greyed, if grey_in_place was asked for)
 * or any other buffer of the batch's frame count and size, in any `format`; after ocvar_hip_render on the same stream the
 * patches show the overlays.  Stream-ordered behind the batch; does not wait.
 * ocvar_hip_patches_records: the same on records the caller supplies in device memory, d_markers [n_frames][records_per_frame]
 * and d_counts [n_frames] (a count above records_per_frame is read as records_per_frame).  Needs no batch; frames of up to the
 * context's max_width x max_height; any n_frames >= 1.  stream NULL: the context's own stream.  Does not wait.
 * Both need no workspace: a context that never asks for patches allocates and launches nothing.  OCVAR_E_ARG, before any device
 * call and with a text in ocvar_hip_last_error, for NULL frames or patches, an unknown format, a row_stride below the format's
 * bytes per pixel times width, a patch side outside 2 .. OCVAR_MAX_PATCH_SIDE, unknown flag bits, records_per_frame outside
 * 1 .. M; ocvar_hip_patches also when nothing is enqueued or width or height differ from the batch's. */
enum { OCVAR_MAX_PATCH_SIDE = 256, OCVAR_PATCH_FLIP_ROWS = 1, OCVAR_PATCH_MATCHED_ONLY = 2 };
int ocvar_hip_patches(OcvarHip* ctx, const uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride, int format,
                      uint8_t* d_patches, int patch_w, int patch_h, int records_per_frame, int flags, int* d_status, void* stream);
int ocvar_hip_patches_records(OcvarHip* ctx, const uint8_t* d_frames, int width, int height, int row_stride, size_t frame_stride,
                              int n_frames, int format, const OcvarMarker* d_markers, const int* d_counts, int records_per_frame,
                              uint8_t* d_patches, int patch_w, int patch_h, int flags, int* d_status, void* stream);

/* Undistortion: frames of a distorting camera, and the marker records found on them, turned into the pinhole world of the same
 * camera matrix without leaving device memory -- what glProjection, ocvar_hip_render* (plain homographies) and ocvar_hip_patches*
 * (straight-edged quads) assume of the frame they are shown over.  The definition, bit for bit, is
 * opencv-ar_amd/csrc/undistort_core.h, with the context's camera (ocvar_hip_set_camera) as it is at the call: fx fy cx cy of
 * cameraMatrix and distCoeffs k1 k2 p1 p2 k3.
 * ocvar_hip_undistort stands for OpenCV's undistort(src, dst, cameraMatrix, distCoeffs, newCameraMatrix = cameraMatrix):
 * destination pixel (u, v) samples the source where the lens model puts the pixel's normalised point, computed in double per
 * pixel (no map is stored), with cvWarpPerspective's 1/32-px bilinear sampling (decode_core.h) and a constant 0 outside the
 * frame.  Every byte of a pixel is remapped alike, byte 3 of a four-channel pixel included.  With all five coefficients zero the
 * frames are copied.
 *   d_src / d_dst  n_frames frames of width x height pixels in `format` (any OCVAR_FMT_*), rows *_row_stride and frames
 *                  *_frame_stride bytes apart, at any address; their byte ranges must not intersect (nothing in place)
 * ocvar_hip_undistort_records stands for undistortPoints(square, cameraMatrix, distCoeffs, R = I, P = cameraMatrix) on the four
 * corners of every record: cvUndistortPoints' five iterations, back to pixels with fx fy cx cy, rounded to float32 (a NaN is
 * stored as 0x7FC00000); with all five coefficients zero the square is copied unchanged.  Every other field is copied as it is, glMatrix included: the pose already
 * accounts for the lens, and its pinhole projection lands on the undistorted corners.
 *   d_markers / d_out  [n_frames][records_per_frame] records (1 <= records_per_frame <= M = ocvar_hip_max_markers(ctx)); slot k
 *                  of frame f is written when k < min(d_counts[f], records_per_frame), no other slot is touched; d_out may be
 *                  d_markers
 * Parity with a real OpenCV build is unpinned: none is at hand where this library is built and tested; the tests pin the host
 * build of undistort_core.h, the agreement of the two maps and detection on undistorted views.
 * Both need no batch and no workspace and can run at any time: a context that never calls them allocates and launches nothing.
 * Frames of up to the context's max_width x max_height; any n_frames >= 1; stream NULL: the context's own stream.  Neither
 * waits.  OCVAR_E_ARG, before any device call and with a text in ocvar_hip_last_error, for NULL pointers, no camera set, fx or fy
 * zero or one of the nine camera numbers not finite, an unknown format, a row stride below the format's bytes per pixel times
 * width, a size above the context's, n_frames < 1, rows that span more than 2^31 - 1 bytes (the rule of
 * ocvar_hip_set_input_format, for source and destination), intersecting byte ranges, records_per_frame outside 1 .. M. */
int ocvar_hip_undistort(OcvarHip* ctx, const uint8_t* d_src, int src_row_stride, size_t src_frame_stride, uint8_t* d_dst,
                        int dst_row_stride, size_t dst_frame_stride, int width, int height, int n_frames, int format, void* stream);
int ocvar_hip_undistort_records(OcvarHip* ctx, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int records_per_frame,
                                OcvarMarker* d_out, void* stream);

/* Flow tracking: marker records carried from a block of previous frames to a block of next frames by sparse pyramidal
 * Lucas-Kanade (the equations of OpenCV's calcOpticalFlowPyrLK) on their four corners, without anything leaving device memory
 * -- the "four points from optical flow" cvarCompareSquare (opencvar.cpp:323-367) expects and nothing in the reference
 * produces.  Two uses: the tracked records as d_prev of ocvar_hip_enqueue_tracked, so that the 20-px rule of cvarTrack compares
 * detections with where the markers are, not where they were; and records and poses carried over frames that are not detected
 * at all.  The definition, bit for bit, is opencv-ar_amd/csrc/flow_core.h: the integer pyramid (the library's grey, OpenCV's
 * 8-bit pyrDown), central differences, float bilinear sampling, sums in double in a fixed order.
 *   d_prev_frames / d_next_frames  n_frames frames of width x height pixels in `format` (any OCVAR_FMT_*), rows *_row_stride and
 *                  frames *_frame_stride bytes apart, at any address; read only.  The two blocks may lie in one buffer at
 *                  different offsets (frame t and t + 1 of a stream, or stream-major blocks).  Flow should see the frames as the
 *                  camera gave them, or the same treatment on both sides: grey_in_place and ocvar_hip_render change frames.
 *   d_markers / d_counts  [n_frames][records_per_frame] records on the previous frames and [n_frames] counts (1 <=
 *                  records_per_frame <= M = ocvar_hip_max_markers(ctx)); slot k of frame f is live when k < min(d_counts[f],
 *                  records_per_frame)
 *   params         NULL: half_win 10, levels 3, max_iter 30, flags 0, eps 0.03, min_eig 1e-3, max_err 0, fb_max 0.  The window
 *                  is (2 half_win + 1)^2 px; the levels used are 0 .. L, L the largest l <= levels whose shorter side is at
 *                  least 2 half_win + 3; min_eig: the smallest eigenvalue of the window's gradient matrix per pixel a corner
 *                  needs; max_err > 0: the largest mean absolute difference of the windows (grey levels) a tracked corner may
 *                  have; fb_max > 0: the corner is tracked back, and may land at most fb_max px from where it started.
 *                  OCVAR_FLOW_POSE: glMatrix of a tracked record is solved from its new square with the context's camera as it
 *                  is at the call (by value) and the record's aspectRatio.
 *   d_out          [n_frames][records_per_frame] records, may be d_markers: a live slot gets the input record with its square
 *                  replaced (status 1), or unchanged (any other status)
 *   d_status       [n_frames][records_per_frame] ints, may be NULL: 1 tracked; the code of the lowest-numbered failing corner: -1
 *                  the corner does not start inside the frame (or is not finite), -2 no texture at level 0, -3 left the frame,
 *                  -4 error above max_err, -5 forward-backward check; -6 all four tracked but the quad is not strictly convex;
 *                  0 the slot is not live -- nothing else of such a slot is touched
 *   d_err          [n_frames][records_per_frame][4] floats, may be NULL: of a live slot the corners' mean absolute differences
 *                  at level 0, -1.0f for a corner that did not get that far
 * Needs no batch and does not wait; stream NULL: the context's own stream.  Frames of up to the context's max_width x
 * max_height with no side below 2 half_win + 3; any n_frames >= 1.  The workspace is allocated by the first call and freed with
 * the context (a context that never calls allocates and launches nothing): two pyramids for each of min(max_batch, 32) frames,
 * a pyramid being the six levels of a max_width x max_height frame with every row rounded up to 64 bytes and the whole to 256
 * -- under 2 (4/3 W H + 2 W + 128 H + 1024) bytes per frame pair; more frames go through it in chunks, in stream order.  Calls of one
 * context that name different streams are ordered by the library (an event behind the last chunk, which the next call's stream
 * waits for), so the workspace is never shared by two calls at once.
 * Parity with a real OpenCV build is unpinned (see ocvar_hip_undistort); the tests pin the host build of flow_core.h, a numpy
 * restatement of the equations and the truth of rendered views.
 * OCVAR_E_ARG, before any device call and with a text in ocvar_hip_last_error, for NULL frames, records, counts or output, an
 * unknown format, a row stride below the format's bytes per pixel times width, rows that span more than 2^31 - 1 bytes (the rule
 * of ocvar_hip_set_input_format), a size above the context's or a side below 2 half_win + 3, n_frames < 1, records_per_frame
 * outside 1 .. M, half_win outside 1 .. OCVAR_MAX_FLOW_HALF_WIN, levels outside 0 .. OCVAR_MAX_FLOW_LEVELS, max_iter outside
 * 1 .. 100, a negative or non-finite eps, min_eig, max_err or fb_max, unknown flag bits, OCVAR_FLOW_POSE without a camera. */
enum { OCVAR_MAX_FLOW_HALF_WIN = 15, OCVAR_MAX_FLOW_LEVELS = 5, OCVAR_FLOW_POSE = 1 };
typedef struct { int half_win, levels, max_iter, flags; float eps, min_eig, max_err, fb_max; } OcvarFlowParams;   /* 32 bytes */
int ocvar_hip_flow_records(OcvarHip* ctx, const uint8_t* d_prev_frames, int prev_row_stride, size_t prev_frame_stride,
                           const uint8_t* d_next_frames, int next_row_stride, size_t next_frame_stride, int width, int height,
                           int n_frames, int format, const OcvarMarker* d_markers, const int* d_counts, int records_per_frame,
                           const OcvarFlowParams* params, OcvarMarker* d_out, int* d_status, float* d_err, void* stream);

/* YUV conversion, the 8-bit limited-range subset (every other range, depth and layout: the _ex calls below): NV12, I420, YUYV and
 * UYVY frames, as a video decoder or a capture card leaves them in
 * device memory, to the interleaved frame formats every other entry point takes, and back for an encoder -- the one full-frame
 * pass of a device-resident decode, detect, draw, encode loop the library did not have.  The definition, bit for bit, is
 * opencv-ar_amd/csrc/yuv_core.h: 20-bit fixed-point integer arithmetic, the chroma sample used as it is (nearest) towards colour,
 * the mean colour of the 2 x 2 (4:2:0) or 2 x 1 (4:2:2) block towards chroma.  ocvar_hip_yuv_to_frames stands for OpenCV's
 * cvtColor with COLOR_YUV2BGR_NV12 / _I420 / _YUY2 / _UYVY (and the RGB, four-channel and grey relatives),
 * ocvar_hip_frames_to_yuv for COLOR_BGR2YUV_I420 and its relatives.
 *   OcvarYuvFrames  layout: OCVAR_YUV_NV12 (a Y plane at y, interleaved U V at c0), OCVAR_YUV_I420 (Y at y, U at c0, V at c1),
 *                  OCVAR_YUV_YUYV (Y0 U Y1 V at y), OCVAR_YUV_UYVY (U Y0 V Y1 at y); plane pointers a layout does not use are
 *                  ignored.  matrix: OCVAR_YUV_BT601 (the constants of OpenCV's YUV family) or OCVAR_YUV_BT709, both limited range
 *                  (Y 16 .. 235, U V 16 .. 240).  y_pitch: bytes between rows of the Y or packed plane; c_pitch: between rows of
 *                  the chroma planes (NV12: at least width, I420: at least width / 2).  Frame f's planes start at plane +
 *                  f * frame_stride, each plane pointer on its own: a decoder surface with a chroma offset fits.  The planes of
 *                  a destination must not overlap each other.
 *   d_dst / d_src  n_frames frames of width x height pixels in `format` (any OCVAR_FMT_*; it need not be the input format), rows
 *                  *_row_stride and frames *_frame_stride bytes apart, at any address.  As a destination BGRA and RGBA get byte
 *                  3 = 255 and GRAY gets the library's grey of the converted colour, so that detection on it is detection on the
 *                  converted BGR frame; as a source byte 3 is ignored and GRAY reads as B = G = R = g.
 * When every plane address, pitch, row stride and frame stride is a multiple of 4 the kernels move whole dwords; otherwise, and
 * in the last pixels of a row, bytes -- with the same result.  No byte outside the pixels and samples is written.
 * Parity with a real OpenCV build is unpinned (see ocvar_hip_undistort): the BT.601 constants are written down from memory of
 * OpenCV; the tests pin the host build of yuv_core.h, a numpy restatement of the equations and the float64 matrices.
 * Both need no batch and no workspace and can run at any time: a context that never calls them allocates and launches nothing.
 * Frames of up to the context's max_width x max_height; any n_frames >= 1 (more than 65535 go in several launches, in stream
 * order); stream NULL: the context's own stream.  Neither waits.  OCVAR_E_ARG, before any device call and with a text in
 * ocvar_hip_last_error, for NULL pointers (of the planes the layout uses), an unknown layout, matrix or format, an odd width, an
 * odd height with NV12 or I420, a size above the context's, n_frames < 1, a pitch below the plane's bytes per row, a row stride
 * below the format's bytes per pixel times width, rows of a plane or of a frame that span more than 2^31 - 1 bytes, byte ranges
 * of a plane and of the frames that intersect (nothing in place). */
enum { OCVAR_YUV_NV12 = 0, OCVAR_YUV_I420 = 1, OCVAR_YUV_YUYV = 2, OCVAR_YUV_UYVY = 3 };
enum { OCVAR_YUV_BT601 = 0, OCVAR_YUV_BT709 = 1 };
typedef struct { int layout, matrix;                    /* OCVAR_YUV_NV12 .., OCVAR_YUV_BT601 / OCVAR_YUV_BT709 */
                 uint8_t* y; uint8_t* c0; uint8_t* c1;  /* Y (or the packed plane); NV12: U V, I420: U; I420: V */
                 int y_pitch, c_pitch; size_t frame_stride; } OcvarYuvFrames;   /* 48 bytes */
int ocvar_hip_yuv_to_frames(OcvarHip* ctx, const OcvarYuvFrames* src, uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride,
                            int width, int height, int n_frames, int format, void* stream);
int ocvar_hip_frames_to_yuv(OcvarHip* ctx, const uint8_t* d_src, int src_row_stride, size_t src_frame_stride, const OcvarYuvFrames* dst,
                            int width, int height, int n_frames, int format, void* stream);

/* YUV conversion of every range, depth and layout: the two calls above are the 8-bit limited-range subset; these take what else
 * arrives in device memory -- the P010 / P012 / P016 surfaces a hardware decoder makes of HEVC Main10, AV1 and VP9 profile 2,
 * the full-range YUV of JPEG and MJPEG, NV21, planar 4:4:4 and the BT.2020 matrix (the matrix only: no transfer function, no tone
 * mapping).  The definition, bit for bit and all integer, is opencv-ar_amd/csrc/yuv_ex_core.h; on every case both pairs of calls
 * accept they write the same bytes.
 *   OcvarYuvFramesEx  layout: the four of OcvarYuvFrames, OCVAR_YUV_NV21 (NV12 with V first in the interleaved plane) and
 *                  OCVAR_YUV_I444 (three planes of full resolution: Y at y, U at c0, V at c1, the chroma rows c_pitch apart; no
 *                  subsampling, so odd widths and heights are taken).  matrix: OCVAR_YUV_BT601, _BT709 or _BT2020.  range:
 *                  OCVAR_YUV_LIMITED (Y 16 .. 235, U V 16 .. 240, times 2^(bits - 8)) or OCVAR_YUV_FULL (0 .. 2^bits - 1); range
 *                  and matrix combine freely.  bits: 8, 10, 12 or 16; above 8 with OCVAR_YUV_NV12 only, which is then P010 / P012 /
 *                  P016: 16-bit little-endian words, the sample word >> (16 - bits), the low bits ignored on read and written as
 *                  zero; pitches stay in bytes, and plane addresses, pitches and frame stride are even.  Everything else as in
 *                  OcvarYuvFrames.
 * Towards colour a limited-range Y below its offset reads as black; towards YUV the limited range is an offset and a scale, not
 * a clamp (Y is held to the sample range only), as in the 8-bit calls.  Chroma towards colour is the sample as it is, chroma from
 * colour the mean colour of the 2 x 2, 2 x 1 or (I444) single pixel.  The frames side, the dword and byte paths (bytes: halfwords
 * for 16-bit samples), the sizes, n_frames, the stream and the refusals are those of the calls above; refused besides: an unknown
 * range or bits, bits > 8 with a layout other than NV12, 16-bit samples at an odd address, pitch or frame stride.  No batch, no
 * workspace, neither waits. */
enum { OCVAR_YUV_NV21 = 4, OCVAR_YUV_I444 = 5 };          /* _ex only */
enum { OCVAR_YUV_BT2020 = 2 };                            /* _ex only */
enum { OCVAR_YUV_LIMITED = 0, OCVAR_YUV_FULL = 1 };
typedef struct { int layout, matrix, range, bits;
                 void* y; void* c0; void* c1;
                 int y_pitch, c_pitch; size_t frame_stride; } OcvarYuvFramesEx;   /* 56 bytes */
int ocvar_hip_yuv_to_frames_ex(OcvarHip* ctx, const OcvarYuvFramesEx* src, uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride,
                               int width, int height, int n_frames, int format, void* stream);
int ocvar_hip_frames_to_yuv_ex(OcvarHip* ctx, const uint8_t* d_src, int src_row_stride, size_t src_frame_stride, const OcvarYuvFramesEx* dst,
                               int width, int height, int n_frames, int format, void* stream);

/* Resizing: device-resident frames brought to another size, and the marker records found at one size carried to the other --
 * a 3840 x 2160 stream is shrunk to 1920 x 1080 for a context of that size (with the camera of cvarCameraScale), and the records
 * it finds are scaled up and drawn on the large frames; previews and thumbnails of rendered frames stay on the device.  The
 * definition, bit for bit, is opencv-ar_amd/csrc/resize_core.h.  ocvar_hip_resize stands for OpenCV's resize(src, dst, dsize, 0,
 * 0, interpolation) on 8-bit images, every byte of a pixel treated alike (byte 3 of a four-channel pixel included):
 *   OCVAR_RESIZE_NEAREST  INTER_NEAREST: source index min(floor(x * scale), s - 1) per axis, scale = 1.0 / ((double)d / s).
 *   OCVAR_RESIZE_LINEAR   INTER_LINEAR of 8-bit images: pixel centres aligned, two 11-bit weights per axis, 32-bit integers.  A
 *                  call whose two scales are exactly 2 gives the AREA result, as in OpenCV.
 *   OCVAR_RESIZE_AREA     INTER_AREA, shrinking only (dst_width <= src_width, dst_height <= src_height, by at most
 *                  OCVAR_MAX_RESIZE_RATIO per axis): the rounded mean of the block when both scales are whole numbers -- the
 *                  2 x 2 block is (sum + 2) >> 2 --, else the fractional coverage table, accumulated in float in a fixed order.
 *   d_src / d_dst  n_frames frames of src_width x src_height and of dst_width x dst_height pixels in `format` (any OCVAR_FMT_*; it
 *                  need not be the input format), rows *_row_stride and frames *_frame_stride bytes apart, at any address; their
 *                  byte ranges must not intersect.  A source rectangle (crop and resize) is d_src moved to the rectangle's first
 *                  pixel with the rectangle's size and the full frame's strides.
 * Sides are 1 .. 32767 on both ends and are NOT bound by the context's max_width x max_height: there is no workspace, and the
 * point is to feed a small context from large frames.  When every address, row stride and frame stride is a multiple of 4 the
 * kernels move whole dwords; otherwise, and in the last pixels of a row, bytes -- with the same result.  No byte outside the
 * destination's pixels is written.
 * ocvar_hip_scale_records carries the four corners of every record from a src_width x src_height frame to a dst_width x
 * dst_height one by the pixel-centre rule of the linear map, (p + 0.5) * ((double)d / s) - 0.5 in double per axis, rounded to
 * float32 (a NaN is stored as 0x7FC00000); on an axis whose extents are equal the coordinate is copied.  Every other field is
 * copied as it is; with OCVAR_SCALE_POSE glMatrix is solved from the new square with the context's camera as it is at the call
 * (by value) -- the camera of the destination size -- and the record's aspectRatio.
 *   d_markers / d_out  [n_frames][records_per_frame] records (1 <= records_per_frame <= M = ocvar_hip_max_markers(ctx)); slot k
 *                  of frame f is written when k < min(d_counts[f], records_per_frame), no other slot is touched; d_out may be
 *                  d_markers
 * Parity with a real OpenCV build is unpinned (see ocvar_hip_undistort): the rules are written down from memory of OpenCV; the
 * tests pin the host build of resize_core.h and a numpy restatement of the rules.
 * Both need no batch and no workspace and can run at any time: a context that never calls them allocates and launches nothing.
 * Any n_frames >= 1 (more than 65535 go in several launches, in stream order); stream NULL: the context's own stream.  Neither
 * waits.  OCVAR_E_ARG, before any device call and with a text in ocvar_hip_last_error, for NULL pointers, an unknown format,
 * interpolation or flag bit, a side outside 1 .. 32767, a row stride below the format's bytes per pixel times width, rows that
 * span more than 2^31 - 1 bytes, n_frames < 1, intersecting source and destination byte ranges, AREA with a destination side
 * above the source's or a source side above OCVAR_MAX_RESIZE_RATIO times the destination's, records_per_frame outside 1 .. M,
 * OCVAR_SCALE_POSE with no camera set. */
enum { OCVAR_RESIZE_NEAREST = 0, OCVAR_RESIZE_LINEAR = 1, OCVAR_RESIZE_AREA = 2, OCVAR_MAX_RESIZE_RATIO = 16, OCVAR_SCALE_POSE = 1 };
int ocvar_hip_resize(OcvarHip* ctx, const uint8_t* d_src, int src_width, int src_height, int src_row_stride, size_t src_frame_stride,
                     uint8_t* d_dst, int dst_width, int dst_height, int dst_row_stride, size_t dst_frame_stride,
                     int n_frames, int format, int interpolation, void* stream);
int ocvar_hip_scale_records(OcvarHip* ctx, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int records_per_frame,
                            int src_width, int src_height, int dst_width, int dst_height, int flags, OcvarMarker* d_out, void* stream);

/* Orientation: device-resident frames turned and mirrored, the marker records found on them carried to the other orientation, and
 * the camera that belongs to the turned frames -- a sideways camera, a clip with a 90 degree display matrix or a mirrored front
 * camera is turned upright before it is detected (the registration is not invariant to the frame's orientation), and the records
 * go back to the frames as they were delivered, without a trip through host memory.  The definition, bit for bit, is
 * opencv-ar_amd/csrc/orient_core.h.  ocvar_hip_orient is a pure permutation of pixels, so OpenCV's rotate, flip and transpose
 * cannot differ from it.  A source pixel or coordinate (x, y) of a src_width x src_height = W x H frame goes to (x', y'):
 *   OCVAR_ORIENT_IDENTITY    (x, y)                  W x H   a copy
 *   OCVAR_ORIENT_ROT90_CW    (H - 1 - y, x)          H x W   rotate(ROTATE_90_CLOCKWISE)
 *   OCVAR_ORIENT_ROT180      (W - 1 - x, H - 1 - y)  W x H   rotate(ROTATE_180)
 *   OCVAR_ORIENT_ROT270_CW   (y, W - 1 - x)          H x W   rotate(ROTATE_90_COUNTERCLOCKWISE)
 *   OCVAR_ORIENT_FLIP_H      (W - 1 - x, y)          W x H   flip(1)
 *   OCVAR_ORIENT_FLIP_V      (x, H - 1 - y)          W x H   flip(0)
 *   OCVAR_ORIENT_TRANSPOSE   (y, x)                  H x W   transpose
 *   OCVAR_ORIENT_TRANSVERSE  (H - 1 - y, W - 1 - x)  H x W   transpose of flip(-1)
 *   d_src / d_dst  n_frames frames of src_width x src_height pixels and of the destination size the table names, in `format` (any
 *                  OCVAR_FMT_*; it need not be the input format), rows *_row_stride and frames *_frame_stride bytes apart, at any
 *                  address; their byte ranges must not intersect (no turning in place, IDENTITY included).  A source rectangle
 *                  is d_src moved to the rectangle's first pixel with the rectangle's size and the full frame's strides.
 * Sides are 1 .. 32767 and are NOT bound by the context's max_width x max_height: there is no workspace.  When every address, row
 * stride and frame stride is a multiple of 4 the kernels move whole dwords; otherwise, and in the last pixels of a row or tile,
 * bytes -- with the same result.  No byte outside the destination's pixels is written; the source is never written.
 * ocvar_hip_orient_records carries the four corners of every record found on a src_width x src_height frame through the table,
 * in double per coordinate, rounded to float32 (a NaN is stored as 0x7FC00000); a coordinate the table passes on unchanged, or
 * only swaps between the axes, is copied bit for bit.  Corner k stays in slot k, so the mirroring orientations (FLIP_H, FLIP_V,
 * TRANSPOSE, TRANSVERSE) reverse the winding of the square.  Every other field is copied as it is; with OCVAR_ORIENT_POSE glMatrix
 * is solved from the new square with the context's camera as it is at the call (by value) -- which must be the camera of the
 * destination orientation: ocvar_hip_orient_camera -- and the record's aspectRatio.  A reflected view has no rigid pose: the flag
 * is refused for the mirroring orientations.
 *   d_markers / d_out  [n_frames][records_per_frame] records (1 <= records_per_frame <= M = ocvar_hip_max_markers(ctx)); slot k
 *                  of frame f is written when k < min(d_counts[f], records_per_frame), no other slot is touched; d_out may be
 *                  d_markers
 * ocvar_hip_orient_camera (host only: no context, no device call) writes the camera of the turned frames: width and height the
 * destination's, fx and fy swapped when the orientation transposes, the principal point through the table (cx' = H - 1 - cy for
 * ROT90_CW), glProjection as cvarCameraScale computes it, k1 k2 k3 kept and (p1, p2) turned with the image plane ((p2, -p1) for
 * ROT90_CW; the full list is in orient_core.h).  out may be in.  OCVAR_E_ARG, with nothing written, for NULL pointers, an unknown
 * orientation, and under any orientation but IDENTITY for a camera matrix that is not fx 0 cx / 0 fy cy / 0 0 1.
 * The two device calls need no batch and no workspace and can run at any time: a context that never calls them allocates and
 * launches nothing.  Any n_frames >= 1 (more than 65535 go in several launches, in stream order); stream NULL: the context's own
 * stream.  Neither waits.  OCVAR_E_ARG, before any device call and with a text in ocvar_hip_last_error, for NULL pointers, an
 * unknown format, orientation or flag bit, a side outside 1 .. 32767, a row stride below the format's bytes per pixel times the
 * width of that side, rows that span more than 2^31 - 1 bytes, n_frames < 1, intersecting source and destination byte ranges,
 * records_per_frame outside 1 .. M, OCVAR_ORIENT_POSE with a mirroring orientation or with no camera set. */
enum { OCVAR_ORIENT_IDENTITY = 0, OCVAR_ORIENT_ROT90_CW = 1, OCVAR_ORIENT_ROT180 = 2, OCVAR_ORIENT_ROT270_CW = 3,
       OCVAR_ORIENT_FLIP_H = 4, OCVAR_ORIENT_FLIP_V = 5, OCVAR_ORIENT_TRANSPOSE = 6, OCVAR_ORIENT_TRANSVERSE = 7,
       OCVAR_ORIENT_POSE = 1 /* flag of ocvar_hip_orient_records */ };
int ocvar_hip_orient(OcvarHip* ctx, const uint8_t* d_src, int src_width, int src_height, int src_row_stride, size_t src_frame_stride,
                     uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride, int n_frames, int format, int orientation, void* stream);
int ocvar_hip_orient_records(OcvarHip* ctx, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int records_per_frame,
                             int src_width, int src_height, int orientation, int flags, OcvarMarker* d_out, void* stream);
int ocvar_hip_orient_camera(const OcvarCamera* in, int orientation, OcvarCamera* out);   /* host only, no context, no device call */

/* Projective warp: device-resident frames mapped by one homography per frame, the marker records carried along, and the maps that
 * show a board's plane from straight above -- a tabletop, a whiteboard, a document or an inspection fixture rectified from the
 * pose ocvar_hip_set_board gives, without a trip through host memory.  The reference's public cvarInvertPerspective(input, output,
 * src, dst) (cvGetPerspectiveTransform + cvWarpPerspective) for any output size and any four points.  The definition, bit for
 * bit, is opencv-ar_amd/csrc/warp_core.h; the sampler is the one ocvar_hip_patches already uses.
 *   d_maps   nine doubles per frame, row by row, in device memory ([n_frames][9]; with OCVAR_WARP_ONE_MAP [9], used for every
 *            frame).  By default the FORWARD map from source pixels to destination pixels, as OpenCV's warpPerspective takes it,
 *            inverted in double (adjugate times 1 / det); with OCVAR_WARP_INVERSE_MAP the nine doubles already map destination
 *            pixels to source pixels.  A frame is SKIPPED when any of its nine numbers is not finite, or when the forward map's
 *            determinant is 0 or its inverse is not finite: d_status[f] = 0 and none of the frame's destination bytes is touched.
 *            Every other frame gets status 1.  d_status ([n_frames] ints, device memory) may be NULL.
 *   pixel    M the destination -> source map.  OCVAR_WARP_LINEAR: cvWarpPerspective's INTER_LINEAR, the source position
 *            ((M0 x + M1 y + M2) / w, (M3 x + M4 y + M5) / w), w = M6 x + M7 y + M8 (w = 0: position 0), fixed to 1/32 px, four taps
 *            under 15-bit weights.  OCVAR_WARP_NEAREST: the source pixel at the position rounded to nearest (ties to even) per
 *            axis.  Every byte of a pixel is treated alike, byte 3 of a four-channel pixel included.
 *   border   OCVAR_WARP_BORDER_CONSTANT: a tap outside the source reads fill[c], four bytes in the format's memory order (fill
 *            NULL: zeros, the rule of ocvar_hip_patches).  OCVAR_WARP_BORDER_REPLICATE: tap coordinates are clamped into the source.
 *   d_src / d_dst  n_frames frames of src_width x src_height and of dst_width x dst_height pixels in `format` (any OCVAR_FMT_*; it
 *            need not be the input format), rows *_row_stride and frames *_frame_stride bytes apart, at any address; their byte
 *            ranges must not intersect.  A source rectangle is d_src moved to the rectangle's first pixel with the rectangle's size
 *            and the full frame's strides (the map then speaks of the rectangle's pixels).
 * Sides are 1 .. 32767 on both ends and are NOT bound by the context's max_width x max_height: there is no workspace.  When the
 * destination's address, row stride and frame stride are multiples of 4 the kernel stores whole dwords; otherwise, and in the
 * last pixels of a row, bytes -- with the same result.  No byte outside the destination's pixels is written, no byte outside the
 * source's pixels is read; the source is never written.
 * ocvar_hip_warp_records carries the four corners of every record through the FORWARD map (OCVAR_WARP_INVERSE_MAP is refused: the
 * records need the forward map) in double, x' = (m0 x + m1 y + m2) / w, rounded once to float32 (a NaN is stored as 0x7FC00000); a
 * corner whose w is 0 or not finite becomes NaN.  Every other field is copied as it is; with OCVAR_WARP_POSE glMatrix is solved
 * from the new square with the context's camera as it is at the call (by value) -- the camera of the warped frames -- and the
 * record's aspectRatio, as ocvar_hip_scale_records does.
 *   d_markers / d_out  [n_frames][records_per_frame] records (1 <= records_per_frame <= M = ocvar_hip_max_markers(ctx)); slot k
 *            of frame f is written when k < min(d_counts[f], records_per_frame), no other slot is touched; d_out may be d_markers
 * ocvar_hip_board_plane_maps writes, for every pose of d_poses [n_frames] (ocvar_hip_board_poses_to_device), the destination ->
 * source map K [r1 r2 t] S -- to be used with OCVAR_WARP_INVERSE_MAP -- of the rectangle rect = (x0, y0, x1, y1) of the board's
 * plane, in board units (host memory, read at the call): K the context's camera matrix as it is at the call, r1 r2 the first two
 * columns of the rotation of rvec, S sending destination pixel (0, 0) to board point (x0, y0) and pixel (dst_width - 1,
 * dst_height - 1) to (x1, y1); the caller flips the picture by choosing y0 > y1.  Sine and cosine of the rotation angle are not
 * the math library's but the definition's own (warp_core.h: warp_sincos, within 1 ulp of them), so that the maps -- which decide
 * bytes -- are the same bits on the device and in the host build.  The lens is ignored: undistort the frames first
 * (ocvar_hip_undistort) and the maps are exact on them.  A pose whose status is not 1, a number that is not finite, or a
 * rectangle of zero extent on an axis whose destination side is above 1 gives nine NaNs, and ocvar_hip_warp then skips that frame
 * (status 0).
 * Parity with a real OpenCV build is unpinned (see ocvar_hip_undistort): the rules are written down from memory of OpenCV; the
 * tests pin the host build of warp_core.h, a numpy restatement of the rules, and the patches' sampler.
 * All three need no batch and no workspace and can run at any time: a context that never calls them allocates and launches
 * nothing.  Any n_frames >= 1 (more than 65535 go in several launches, in stream order); stream NULL: the context's own stream.
 * None waits.  OCVAR_E_ARG, before any device call and with a text in ocvar_hip_last_error, for NULL pointers (fill and d_status
 * may be NULL), an unknown format, interpolation, border or flag bit, a side outside 1 .. 32767, a row stride below the format's
 * bytes per pixel times width, rows that span more than 2^31 - 1 bytes, n_frames < 1, intersecting source and destination byte
 * ranges, records_per_frame outside 1 .. M, OCVAR_WARP_POSE or ocvar_hip_board_plane_maps with no camera set,
 * OCVAR_WARP_INVERSE_MAP given to ocvar_hip_warp_records. */
enum { OCVAR_WARP_NEAREST = 0, OCVAR_WARP_LINEAR = 1,
       OCVAR_WARP_BORDER_CONSTANT = 0, OCVAR_WARP_BORDER_REPLICATE = 1,
       OCVAR_WARP_INVERSE_MAP = 1, OCVAR_WARP_ONE_MAP = 2,   /* flags of ocvar_hip_warp / _warp_records */
       OCVAR_WARP_POSE = 4 };                                /* flag of ocvar_hip_warp_records */
int ocvar_hip_warp(OcvarHip* ctx, const uint8_t* d_src, int src_width, int src_height, int src_row_stride, size_t src_frame_stride,
                   uint8_t* d_dst, int dst_width, int dst_height, int dst_row_stride, size_t dst_frame_stride, int n_frames, int format,
                   const double* d_maps, int interpolation, int border, const uint8_t fill[4], int flags, int* d_status, void* stream);
int ocvar_hip_warp_records(OcvarHip* ctx, const OcvarMarker* d_markers, const int* d_counts, int n_frames, int records_per_frame,
                           const double* d_maps, int flags, OcvarMarker* d_out, void* stream);
int ocvar_hip_board_plane_maps(OcvarHip* ctx, const OcvarBoardPose* d_poses, int n_frames, const double rect[4], int dst_width,
                               int dst_height, double* d_maps, void* stream);

/* Levels: the grey levels of device-resident frames stretched, for the whole frame or per tile with the maps of neighbouring tiles
 * blended, into one GRAY plane per frame -- an under-exposed, washed-out or unevenly lit stream brought back to where the
 * detection's fixed thresholds (the adaptive threshold's constant 8 and the cut at grey 100 on the warped patch, reference
 * opencvar.cpp:181 and :724) find its markers, without a trip through host memory.  The definition, bit for bit and all integer,
 * is opencv-ar_amd/csrc/levels_core.h.  It is the library's own rule: there is no OpenCV function to be in parity with; with
 * low_ppm = high_ppm = 0 and no gain cap reached it is normalize(..., NORM_MINMAX) up to rounding.
 *   d_src    n_frames frames of width x height pixels in `format` (any OCVAR_FMT_*; it need not be the input format), rows
 *            src_row_stride and frames src_frame_stride bytes apart, at any address.  g is the library's grey of a pixel,
 *            (1868 B + 9617 G + 4899 R + 8192) >> 14 with the format's channel order, the byte itself for GRAY.
 *   d_dst    one GRAY plane of width x height bytes per frame, rows dst_row_stride and planes dst_frame_stride bytes apart, at any
 *            address; the byte ranges of the two sides must not intersect.  Detected with ocvar_hip_set_input_format(OCVAR_FMT_GRAY)
 *            the plane yields records in the source frame's own coordinates: nothing needs carrying across, and drawing
 *            (ocvar_hip_annotate_records, ocvar_hip_render_records) goes onto the original frames.
 *   params   tiles_x, tiles_y  1 .. 16 each, tiles_x tiles_y <= 64, tiles_x <= width, tiles_y <= height (default 1, 1: one map per
 *                              frame); low_ppm, high_ppm  0 .. 500000, the parts per million of a tile's pixels clipped at the dark
 *            and at the bright end (default 10000 each: 1 %); max_gain_q8  256 .. 65280, the largest gain in 1/256 (default 2048:
 *            8).  NULL: the defaults, which ocvar_hip_levels_default_params (host only) writes.
 *   tiles    edges xe[i] = (i width) / tiles_x and ye[j] = (j height) / tiles_y by floor division; tile (j, i) owns the pixels
 *            xe[i] <= x < xe[i+1], ye[j] <= y < ye[j+1], n in all; its histogram is the 256 counts of g over them.
 *   LUT      per tile: k_lo = (n low_ppm) / 1000000 and k_hi = (n high_ppm) / 1000000 in 64 bits; lo the smallest v with
 *            #{g <= v} > k_lo, hi the largest v with #{g >= v} > k_hi; minr = (255 * 256 + max_gain_q8 - 1) / max_gain_q8; if
 *            hi - lo < minr (which also covers lo > hi): lo = min(max((lo + hi - minr) >> 1, 0), 255 - minr) with an arithmetic
 *            shift and hi = lo + minr.  lut[v] = clamp(((v - lo) 510 + (hi - lo)) / (2 (hi - lo)), 0, 255), a floor division of a
 *            value that is made 0 when negative.
 *   blend    between tile centres.  Along x for pixel x: c2[i] = xe[i] + xe[i+1], p = 2 x + 1, i0 the largest i with c2[i] <= p
 *            clamped to 0 .. max(tiles_x - 2, 0), i1 = min(i0 + 1, tiles_x - 1), wx = i1 > i0 ? clamp(((p - c2[i0]) 256) /
 *            (c2[i1] - c2[i0]), 0, 256) : 0; along y the same with ye, giving j0, j1 and wy.  top = lut[j0][i0][g] (256 - wx) +
 *            lut[j0][i1][g] wx, bot the same on row j1, and the output byte is (top (256 - wy) + bot wy + 32768) >> 16.  With one
 *            tile it is lut[g].
 * Three kernels in stream order: histograms (32-bit integer adds, which commute: the result does not depend on scheduling), one
 * LUT per tile, the blend.  Sides are 1 .. 32767 and are NOT bound by the context's max_width x max_height.  When every address,
 * row stride and frame stride is a multiple of 4 the kernels move whole dwords; otherwise, and at the ends of rows and tiles,
 * bytes -- with the same result.  No byte outside the destination's pixels is written; the source is never written.
 * The workspace -- histograms and LUTs of 64 tiles for each of 256 frames, 20 MiB -- is allocated by the first call: a context
 * that never calls ocvar_hip_levels allocates and launches nothing.  More than 256 frames go in several rounds in stream order.
 * Calls of one context share the workspace: like ocvar_hip_annotate_records, a call on another stream than the previous one is
 * ordered behind it by the library, and calls of one context come from one thread at a time.  stream NULL: the context's own
 * stream.  The call does not wait.  OCVAR_E_ARG, before any device call and with a text in ocvar_hip_last_error, for NULL
 * pointers (params may be NULL), an unknown format, a side outside 1 .. 32767, a row stride below the bytes per pixel times
 * width (the destination: below width), rows that span more than 2^31 - 1 bytes, n_frames < 1, intersecting source and
 * destination byte ranges, any parameter outside its range above. */
typedef struct OcvarLevelsParams {
    int tiles_x, tiles_y, low_ppm, high_ppm, max_gain_q8;
} OcvarLevelsParams;
int ocvar_hip_levels_default_params(OcvarLevelsParams* params);   /* host only, no context, no device call */
int ocvar_hip_levels(OcvarHip* ctx, const uint8_t* d_src, int width, int height, int src_row_stride, size_t src_frame_stride,
                     int format, uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride, int n_frames,
                     const OcvarLevelsParams* params, void* stream);

/* Bayer: the raw mosaic of a machine-vision camera (GigE, USB3, CSI), in 8-bit bytes or in 16-bit words holding 9 .. 16 bits,
 * demosaiced on the device into frames of any OCVAR_FMT_*, behind a black level and a white balance -- what render, annotate,
 * patches, warp and ocvar_hip_frames_to_yuv need of such a camera's frames.  The definition, bit for bit and all integer, is
 * opencv-ar_amd/csrc/bayer_core.h.  The call stands for OpenCV's cvtColor with COLOR_Bayer*2BGR and its relatives (bilinear); no
 * OpenCV exists where this library is built and tested, so parity with an OpenCV build is unpinned and not claimed, and the border
 * rule is the library's own.
 *   pattern   named by the colours of the top-left 2 x 2 block, row by row: OCVAR_BAYER_RGGB, _GRBG, _GBRG, _BGGR.  (OpenCV names
 *             its constants by the second row's 2 x 2: COLOR_BayerBG2BGR is RGGB.)  A source rectangle is d_src moved to its first
 *             sample with the full frame's strides and the pattern ocvar_hip_bayer_pattern_at(pattern, x0, y0) of its origin.
 *   bits      8: one byte per sample.  9 .. 16: one little-endian 16-bit word per sample, right-aligned, the sample being
 *             word & (2^bits - 1); MSB-aligned data is read with bits = 16.  A 16-bit source has an even address and even strides.
 *   black, gain_b, gain_g, gain_r   on each sample, with the gain of the sample's own colour (1024 = 1.0), before interpolation:
 *             s' = min(2^bits - 1, (max(s - black, 0) gain + 512) >> 10); black 0 .. 2^bits - 1, gains 0 .. 16383.
 *   interpolation  at an R or B site: own colour = the sample, G = (N + S + W + E + 2) >> 2, the opposite colour = (NW + NE + SW +
 *             SE + 2) >> 2; at a G site: G = the sample, the colour of the row's other sites = (W + E + 1) >> 1, of the column's
 *             = (N + S + 1) >> 1.  A coordinate outside the frame is reflected without repeating the edge (-1 -> 1, W -> W - 2),
 *             which keeps the colour phase: a mosaic of one colour gives that colour everywhere.
 *   reduction for bits > 8: v8 = min(255, (v + (1 << (bits - 9))) >> (bits - 8)).
 *   d_dst     n_frames frames of width x height pixels in `format`; BGRA and RGBA get byte 3 = 255, GRAY the library's grey of the
 *             demosaiced colour, (1868 B + 9617 G + 4899 R + 8192) >> 14: detection on it is detection on the demosaiced BGR frame.
 * params NULL: the defaults (RGGB, 8 bits, black 0, gains 1024), which ocvar_hip_bayer_default_params (host only) writes.  Sides
 * are 2 .. 32767, odd ones included, and are NOT bound by the context's max_width x max_height.  When every address, row stride and
 * frame stride of both sides is a multiple of 4 the kernels move whole dwords; otherwise, and at the ends of rows, bytes -- with the
 * same result.  No byte outside the destination's pixels is written; the source is never written.  No workspace: the call
 * allocates nothing and does not wait.  More than 65535 frames go in several launches, in order.  stream NULL: the context's own
 * stream.  OCVAR_E_ARG, before any device call and with a text in ocvar_hip_last_error, for a NULL pointer (params may be NULL), a
 * side below 2 or above 32767, an unknown pattern or format, bits outside 8 .. 16, black or a gain out of range, a row stride below
 * the row's bytes, rows that span more than 2^31 - 1 bytes, a 16-bit source at an odd address or with an odd stride, n_frames < 1,
 * intersecting source and destination byte ranges. */
enum { OCVAR_BAYER_RGGB = 0, OCVAR_BAYER_GRBG = 1, OCVAR_BAYER_GBRG = 2, OCVAR_BAYER_BGGR = 3 };
typedef struct { int pattern, bits, black, gain_b, gain_g, gain_r; } OcvarBayerParams;   /* 24 bytes */
int ocvar_hip_bayer_default_params(OcvarBayerParams* p);             /* host only: RGGB, 8, 0, 1024 x 3 */
int ocvar_hip_bayer_pattern_at(int pattern, int x0, int y0);         /* host only; -1 for an unknown pattern */
int ocvar_hip_bayer_to_frames(OcvarHip* ctx, const void* d_src, int src_row_stride, size_t src_frame_stride,
                              uint8_t* d_dst, int dst_row_stride, size_t dst_frame_stride,
                              int width, int height, int n_frames, int format, const OcvarBayerParams* params, void* stream);

/* Batch detection on frames already resident in device memory.
 *   d_bgr        frames in the context's input format (default 8UC3 interleaved BGR: ocvar_hip_set_input_format), frame f
 *                starts at d_bgr + f*frame_stride, rows row_stride bytes apart
 *   grey_in_place non-zero: overwrite each frame with its grey version (the reference's side effect,
 *                opencvar.cpp:624-627)
 *   prev / prev_counts  host arrays [n_frames][M] (M = ocvar_hip_max_markers(ctx): OCVAR_MAX_MARKERS unless the context
 *                is dense) and [n_frames] of the previous call's markers per stream, or NULL for stateless detection
 *   markers / counts    host outputs [n_frames][max_per_frame] and [n_frames]; counts[f] is the reference's
 *                return value for frame f (may exceed max_per_frame; only the first max_per_frame are stored)
 * ocvar_hip_detect_device = enqueue + wait + copy-out.  The enqueue/collect pair lets a caller time or
 * overlap the device work; `stream` is a hipStream_t (NULL = the context's own stream). */
int ocvar_hip_detect_device(OcvarHip* ctx, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride,
                            int n_frames, int grey_in_place, const OcvarMarker* prev, const int* prev_counts,
                            OcvarMarker* markers, int* counts, int max_per_frame);
int ocvar_hip_enqueue(OcvarHip* ctx, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride,
                      int n_frames, int grey_in_place, const OcvarMarker* prev, const int* prev_counts, void* stream);
int ocvar_hip_collect(OcvarHip* ctx, OcvarMarker* markers, int* counts, int max_per_frame);
/* ocvar_hip_enqueue with the previous markers in DEVICE memory: d_prev [n_frames][M], d_prev_counts [n_frames]
 * (M = ocvar_hip_max_markers(ctx); counts above M are read as M), e.g. the block ocvar_hip_results_to_device wrote for the
 * same streams one time step earlier -- the tracking state of a block of video streams (the caller-owned `markers` vector of
 * cvarArMultRegistration, /root/reference/src/opencvar.cpp:635-668, samples/ARTest.cpp:57) then never leaves the device.
 * The copy into the context is stream-ordered: the arrays may be overwritten by ocvar_hip_results_to_device of the same
 * batch. */
int ocvar_hip_enqueue_tracked(OcvarHip* ctx, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride,
                              int n_frames, int grey_in_place, const OcvarMarker* d_prev, const int* d_prev_counts, void* stream);
/* 1 if the enqueued batch has finished (ocvar_hip_collect will not wait), 0 if it is still running, < 0 on error or when
 * nothing is enqueued.  A caller with several contexts in flight collects the one that is ready first. */
int ocvar_hip_ready(OcvarHip* ctx);
/* How many marker records per frame a batch brings to the host (1 .. M = ocvar_hip_max_markers(ctx), the default): the copy-out of a
 * 2048-frame batch is 24 MB at 64 records per frame, 3 MB at 8.  ocvar_hip_collect returns at most this many per frame;
 * the counts are always the frames' full counts. */
int ocvar_hip_set_result_limit(OcvarHip* ctx, int max_per_frame);

/* Launch parameters that change how the work is cut, never what comes out (every value gives bit-identical results; the
 * defaults are the measured optimum for the batch size).  value 0 restores the default.  The product library reads no tuning
 * from the environment; only builds made with -DOCVAR_PROF (`make prof`) also honour OCVAR_* variables of the same names. */
enum { OCVAR_TUNE_CROP_PHASES = 1, /* crop-pass tier 2 in 1 launch or 2 (exact pruning behind the crop's best quad) */
       OCVAR_TUNE_MID_STEPS = 2,   /* step budget of follower tier 2 before a border goes to the wave tier (>= 32) */
       OCVAR_TUNE_MID_BLOCKS = 3, OCVAR_TUNE_LONG_BLOCKS = 4, OCVAR_TUNE_SHORT_BLOCKS = 5, /* grids of tiers 2, 3, 1 */
       OCVAR_TUNE_MIN_UNITS = 6,   /* binarise work units per launch below which row chunks are not made taller */
       OCVAR_TUNE_GATE_MODE = 8,   /* which of a context's two binarise kernels wait at its gate: 0 both (default), 1 the frames
                                    * kernel only, 2 the crops kernel only */
       OCVAR_TUNE_WARP_DIRECT = 9, /* 1: every tile of ocvar_hip_warp reads the source directly, none is staged through LDS */
       OCVAR_TUNE_BAYER_PAIRS = 10, /* row pairs a lane of ocvar_hip_bayer_to_frames marches down, 1 .. 64 (default 4) */
       OCVAR_TUNE_HP_MASK = 7 };   /* kernels launched on the context's high-priority stream, one bit per launch: 1 tier 1
                                    * (frames), 2 tier 2, 4 tier 3, 8 order/crops, 16 tier 1 (crops), 32 tier 2, 64 tier 3,
                                    * 128 decode, 256 dedupe+pose; ocvar_hip_set_tuning(ctx, OCVAR_TUNE_HP_MASK, m) sets mask m
                                    * (0 = none), there is no "back to default" for this knob short of a new context */
int ocvar_hip_set_tuning(OcvarHip* ctx, int knob, int value);
/* How the library was built: "... product(...)" or "... OCVAR_PROF(...)" -- bench.py prints it with its number. */
const char* ocvar_hip_build_info(void);

/* The context's own HIP stream (hipStream_t), for callers that order their own work or events against a batch.  It is what
 * ocvar_hip_enqueue uses when its `stream` argument is NULL and the context has no gate.  With a gate the batch runs on one of
 * the gate's lanes, and the stream keeps these promises: work that is on it when ocvar_hip_enqueue is called (a kernel that
 * writes the frames, a wait for an event) precedes the batch; ocvar_hip_results_to_device / ocvar_hip_board_poses_to_device
 * that name it follow the batch -- they run on the batch's lane, like those that name no stream --, and ocvar_hip_collect
 * returns only when such a copy has arrived (a gather may read the block right after collect).  Other work put on the stream
 * after the enqueue is NOT ordered behind the batch or those copies (that would take a wait in a hardware queue the stream
 * shares with a lane): wait for ocvar_hip_collect, or name a stream in ocvar_hip_enqueue.  ocvar_hip_collect does not wait for
 * whatever else is on the lane that carried the batch. */
void* ocvar_hip_stream(const OcvarHip* ctx);

/* After ocvar_hip_enqueue: stream-ordered device-to-device copy of the batch's results into caller-owned device
 * buffers, d_markers [n_frames][M] (M = ocvar_hip_max_markers(ctx)) and d_counts [n_frames] -- for callers that gather results
 * across GPUs (RCCL) before any host copy.  Does not wait; ocvar_hip_collect must still be called. */
int ocvar_hip_results_to_device(OcvarHip* ctx, OcvarMarker* d_markers, int* d_counts, void* stream);
/* Same with a narrower block: d_markers [n_frames][max_per_frame] (1 <= max_per_frame <= M) holds the first
 * max_per_frame records of every frame; d_counts still carries the frames' full counts, so a frame with more markers than
 * the block keeps is visible to the receiver.  A gather of 8 records per frame moves 1/8 of the bytes over xGMI. */
int ocvar_hip_results_to_device_ex(OcvarHip* ctx, OcvarMarker* d_markers, int* d_counts, int max_per_frame, void* stream);

/* Several contexts on one GPU as one detector: n_contexts contexts of chunk_frames frames each (own streams, one shared gate
 * of gate_width binarise kernels, 0: none) detect a device-resident array of any number of frames chunk by chunk, every context
 * with one chunk in flight (csrc/pipe.hip: the schedule of bench.py behind the C ABI -- four or five contexts, gate 2: ~1.9x the
 * frames/s of one context).  Stateless; results in frame order like ocvar_hip_detect_device.  No counterpart in the reference
 * (one frame per call); the many-frames form of its per-frame loop, samples/ARTest.cpp:43-82. */
typedef struct OcvarPipe OcvarPipe;
int ocvar_hip_pipe_create(OcvarPipe** pipe, int device, int max_width, int max_height, int chunk_frames, int n_contexts, int gate_width);
void ocvar_hip_pipe_destroy(OcvarPipe* pipe);
const char* ocvar_hip_pipe_last_error(const OcvarPipe* pipe);
int ocvar_hip_pipe_set_templates(OcvarPipe* pipe, const OcvarTemplate* templates, int n);
int ocvar_hip_pipe_set_camera(OcvarPipe* pipe, const OcvarCamera* camera);
int ocvar_hip_pipe_detect_device(OcvarPipe* pipe, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride,
                                 long long n_frames, int grey_in_place, OcvarMarker* markers, int* counts, int max_per_frame);
/* Stateful form (the reference's behaviour over video: `markers` persists across calls, opencvar.cpp:635-668): one call = one
 * time step of n_streams video streams, frame s of d_bgr being stream s's current frame.  Every stream's markers of the
 * previous step are its tracking input; they are kept by the pipe in device memory between calls (never copied to the host
 * and back).  reset != 0 (or a different n_streams than the last call): the streams start with no markers, i.e. a stateless
 * first step.  Streams are independent, so chunks of streams go round the contexts as chunks of frames do above; results in
 * stream order. */
int ocvar_hip_pipe_track_device(OcvarPipe* pipe, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride,
                                long long n_streams, int grey_in_place, int reset, OcvarMarker* markers, int* counts, int max_per_frame);

/* Streaming form for a caller with an endless supply of frames (the many-cameras form of the reference's per-frame loop,
 * samples/ARTest.cpp:43-82): the pipeline of contexts is kept full instead of being filled and drained per call.  submit hands
 * a chunk of n_frames <= chunk_frames device-resident frames to the next context and returns at once (OCVAR_E_BUSY when every
 * context already has a chunk in flight); collect waits for the OLDEST chunk in flight, writes its markers [n][max_per_frame]
 * and counts [n], stores the tag it was submitted under and returns its frame count n (0: nothing in flight, < 0: error).
 * Stateless.  set_result_limit (only while nothing is in flight; 1..OCVAR_MAX_MARKERS, default OCVAR_MAX_MARKERS): how many
 * marker records per frame the submitted chunks bring to the host, as ocvar_hip_set_result_limit.  collect returns OCVAR_E_ARG,
 * and leaves the chunk in flight, when max_per_frame exceeds that limit (rows the chunk never brought back).  The markers
 * buffer must hold n rows of max_per_frame records, n up to chunk_frames.  detect_device / track_device bring back
 * max_per_frame records per frame for their own call and leave the limit as it was; they fail with OCVAR_E_ARG while a
 * submitted chunk is in flight. */
enum { OCVAR_E_BUSY = -6 };
int ocvar_hip_pipe_submit(OcvarPipe* pipe, uint8_t* d_bgr, int width, int height, int row_stride, size_t frame_stride, int n_frames,
                          int grey_in_place, long long tag);
int ocvar_hip_pipe_collect(OcvarPipe* pipe, long long* tag, OcvarMarker* markers, int* counts, int max_per_frame);
int ocvar_hip_pipe_in_flight(const OcvarPipe* pipe);
int ocvar_hip_pipe_set_result_limit(OcvarPipe* pipe, int max_per_frame);
/* The input format of every context of the pipe (ocvar_hip_set_input_format), for detect_device, submit and track_device.
 * OCVAR_E_ARG for an unknown format or while a submitted chunk is in flight. */
int ocvar_hip_pipe_set_input_format(OcvarPipe* pipe, int format);
/* ocvar_hip_set_corner_refine on every context of the pipe.  OCVAR_E_ARG outside its ranges or while a submitted chunk is in
 * flight. */
int ocvar_hip_pipe_set_corner_refine(OcvarPipe* pipe, int half_win, int max_iter, float eps);

/* Same, frames in host memory, h_bgr in the context's input format (copied over PCIe first; greyed frames are copied back
 * when requested -- never in OCVAR_FMT_GRAY, where the frames are their own grey). */
int ocvar_hip_detect_host(OcvarHip* ctx, uint8_t* h_bgr, int width, int height, int row_stride, size_t frame_stride,
                          int n_frames, int grey_in_place, const OcvarMarker* prev, const int* prev_counts,
                          OcvarMarker* markers, int* counts, int max_per_frame);

/* cvarFindSquares on one 8-bit single-channel host image (the reference runs it on grey 3-channel images
 * whose channels are equal).  quads: up to max_quads x 8 ints in the reference's sequence order. */
int ocvar_hip_find_squares(OcvarHip* ctx, const uint8_t* h_gray, int width, int height, int row_stride, int* quads,
                           int max_quads, int* n_quads);

/* Parity hooks on the state left by the last detect/enqueue+collect call. */
int ocvar_hip_debug_gray(OcvarHip* ctx, int frame, uint8_t* h_gray /* width*height */);
int ocvar_hip_debug_binary(OcvarHip* ctx, int frame, uint8_t* h_bin /* (w&~1)*(h&~1), values 0/255 */);
/* the frame pass's 8-neighbour masks, untiled: bit s of pixel (x,y) = the neighbour in direction s (0..7 = E,NE,N,NW,W,SW,S,SE) is set */
int ocvar_hip_debug_masks(OcvarHip* ctx, int frame, uint8_t* h_masks /* (w&~1)*(h&~1) */);
int ocvar_hip_debug_frame_quads(OcvarHip* ctx, int frame, int* quads /* OCVAR_MAX_QUADS*8 */, int* n_quads);
/* the pre-dedupe candidates in the reference's order (square-major, all templates of every square with a crop quad); at most
 * max_cands are written, *n_cands is the full count */
int ocvar_hip_debug_candidates(OcvarHip* ctx, int frame, OcvarCandidate* cands, int max_cands, int* n_cands);
/* The crop pass of the last collected batch: the rectangle around every frame-pass square (grown by 5 px, clipped by the frame)
 * that the second pass binarises and searches on its own.  index: the ROI's place in the batch's list (the order is not
 * defined: the squares of a batch append concurrently); owner: the index of the frame-pass square (ocvar_hip_debug_frame_quads)
 * within `frame`; x0, y0, w, h: the rectangle in frame pixels.  ocvar_hip_debug_crop_rois writes the first max_rois records
 * and stores the full count, which is at most the context's ROI capacity (max_batch x squares per frame).
 * ocvar_hip_debug_crop_plane expands the bit plane of ROI `roi` to a byte per pixel, (w & ~1) x (h & ~1) bytes: masks == 0 the
 * binary image (0 / 255, the 1-px frame zero) as ocvar_hip_debug_binary gives a frame's, else the 8-neighbour masks as
 * ocvar_hip_debug_masks.  Both copy out of the workspace and launch nothing; they are valid from ocvar_hip_collect (or a
 * detect call) until the context's next enqueue, and return OCVAR_E_ARG for a bad index, while a batch is in flight, and when
 * no batch with a crop pass has been collected. */
typedef struct OcvarCropRoi {
    int index, frame, owner, x0, y0, w, h;
} OcvarCropRoi;
int ocvar_hip_debug_crop_rois(OcvarHip* ctx, OcvarCropRoi* rois, int max_rois, int* n_rois);
int ocvar_hip_debug_crop_plane(OcvarHip* ctx, int roi, int masks, uint8_t* h_plane /* (w&~1)*(h&~1) */);

/* The border starts of the last collected batch: the list the binarise kernel of the frame pass (crop_pass == 0) or of the crop
 * pass (crop_pass != 0) handed to the border followers -- every pixel at which a border can begin, found from the pixel's
 * neighbours alone.  roi: the frame's index in the batch, or the crop's index in ocvar_hip_debug_crop_rois' list; x, y: the
 * pixel in that frame's or crop's binary image; is_hole: 1 for the start of a hole border.  The order of the list differs from
 * run to run.  Writes the first max_starts records and stores the full count (what ocvar_hip_counters reports in slots 0 and 3,
 * clamped to the list's capacity).  Copies out of the workspace and launches nothing; valid like ocvar_hip_debug_crop_rois, and
 * for crop_pass != 0 only after a batch that ran the crop pass. */
typedef struct OcvarStart {
    int roi, x, y, is_hole;
} OcvarStart;
int ocvar_hip_debug_starts(OcvarHip* ctx, int crop_pass, OcvarStart* starts, int max_starts, int* n_starts);

/* The ring verdicts of the last collected batch, one int per frame (crop_pass == 0, indexed by the frame's place in the batch)
 * or per crop ROI (crop_pass != 0, indexed like ocvar_hip_debug_crop_rois' `index`): 1 where the ring of pixels next to the zeroed
 * 1-px frame of the frame's or crop's binary image -- rows 1 and sh-2, columns 1 and sw-2 -- is all set and both sides are at
 * least 8, so that the border which begins at (1, 1) is dropped without a walk; else 0.  Only batches of more than 8 frames
 * judge their rings: a batch of at most 8 frames gives all zeros.  Writes the first max_flags values and stores the full count
 * (the batch's frames, or its crop ROIs).  Copies out of the workspace and launches nothing; valid and refused like
 * ocvar_hip_debug_starts. */
int ocvar_hip_debug_rings(OcvarHip* ctx, int crop_pass, int* flags, int max_flags, int* n_flags);

/* Measurement aid: runs a dword-per-lane copy of `bytes` bytes (the binarise kernel's access widths) so that a
 * rocprofv3 PMC pass can calibrate FETCH_SIZE / WRITE_SIZE for that pattern (tools/collect_traffic.py). */
int ocvar_hip_debug_calibrate(OcvarHip* ctx, size_t bytes);

/* Per-kernel device time of the last enqueue in milliseconds (HIP events on the launch stream), 12 entries:
 * [0] binarise(frames) [1..3] follower tiers 1,2,3 (frames) [4] order/crops [5] binarise(crops)
 * [6..8] follower tiers 1,2,3 (crops) [9] decode [10] dedupe+pose [11] whole batch.  Returns the number written. */
int ocvar_hip_stage_ms(OcvarHip* ctx, float* ms, int n);
/* The same 13 stage boundaries ([0] start of binarise(frames) ... [12] end of the copy-out) as milliseconds after ref_event, a
 * hipEvent_t the caller recorded (with timing) on this device before enqueueing: stamps of different contexts are on one clock,
 * so a caller with several contexts in flight can tell how launches of one kernel overlapped.  Returns the number written. */
int ocvar_hip_stage_stamps(OcvarHip* ctx, void* ref_event, float* ms, int n);
/* Work counters of the last batch: [0] frame start candidates [1] crop ROIs [2] crop tiles
 * [3] crop start candidates [4] sum of crop areas (pixels) [5] point-pool ints used [6],[7] starts handed to follower
 * tier 2 (frames, crops) [8],[9] borders handed to tier 3 (frames, crops) [10]..[41] profiling slots of builds made with
 * -DOCVAR_PROF (tools/prof_tier2.py), zero in the product build. */
int ocvar_hip_counters(OcvarHip* ctx, long long* out, int n);

#ifdef __cplusplus
}
#endif
#endif
