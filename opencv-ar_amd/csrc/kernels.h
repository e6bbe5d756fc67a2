// kernels.h -- device workspace layout and launch entry points shared by the .hip translation units.
#pragma once
#include "hd.h"
#include "frames_core.h"
#include "decode_core.h"
#include "pose_core.h"
#include "tail_core.h"
#include "refine_core.h"
#include "board_core.h"
#include "overlay_core.h"
#include "annotate_core.h"
#include "patch_core.h"
#include "undistort_core.h"
#include "yuv_core.h"
#include "yuv_ex_core.h"
#include "resize_core.h"
#include "orient_core.h"
#include "warp_core.h"
#include "levels_core.h"
#include "bayer_core.h"
#include "flow_core.h"
#include "croplist_core.h"
#include "ocvar_hip.h"

namespace ocvar {

constexpr int MAXQ_DEFAULT = OCVAR_MAX_QUADS;   // frame-pass quads kept per frame unless the context was created for more (Workspace::maxq)
constexpr int MAXM = OCVAR_MAX_MARKERS;    // markers kept per frame (tracked + new) unless the context was created for more (Workspace::maxm)
constexpr int MAXT = OCVAR_MAX_TEMPLATES;
constexpr int MARCH_HALO_L = 2, MARCH_HALO_R = 2;   // halo lanes (4 pixels each) left / right of a strip's output lanes
constexpr int MARCH_STRIP = 4 * (64 - MARCH_HALO_L - MARCH_HALO_R);   // 240 output columns of one wave's strip in the binarise kernel (256 loaded)
static_assert(MARCH_STRIP == GRAY_PANEL_COLS && 4 * MARCH_HALO_L == GRAY_PANEL_LEAD && 4 * 64 == GRAY_PANEL_BYTES, "a grey panel is what one wave of the frame kernel converts");
constexpr int MARCH_CROP_ROWS = 252;       // rows per work unit in the crop pass (whole tile rows of the bit plane: a multiple of 14)
constexpr int MARCH_STAGE = 512;           // border starts a wave stages in LDS between two appends to the global list
constexpr int BACK_STEPS = 32;             // backward look of an outer start before it follows its border
constexpr int PRE_STEPS = 8;               // steps every plausible start gets before it may queue for tier 1's full budget
constexpr int SHORT_STEPS = 96;            // step budget of follower tier 1 (every plausible start, one lane each)
constexpr int MID_STEPS = 1536;            // step budget of tier 2 (borders that outlived tier 1, one lane each); the rest: tier 3, one wave each
constexpr int CROP_STEPS_CAP = 3072;       // most steps a walk of the crop pass gets in tier 2 in a throughput batch (croplist_core.h: crop_walk_budget)
constexpr int SLAB_PTS = 1024;             // points (packed x | y << 16) a tier-2 lane can keep in its private slab (no second follow needed below that)
constexpr int SLAB_STRIDE = SLAB_PTS + 4;  // dwords per tier-2 lane slab: the points + the scratch slot of flat_step
constexpr int MID_BLOCKS_MAX = 1024;       // tier-2 grid limit (x256 threads, one slab each)
constexpr int SLAB3_PTS = 8192;            // points a tier-3 wave can keep in its slab
constexpr int SLAB3_STRIDE = SLAB3_PTS + 64;   // dwords per tier-3 wave slab
constexpr int LONG_BLOCKS_MAX = 1024;      // tier-3 grid limit (x4 waves, one slab each)

// error bits accumulated in Workspace::err[0]
enum { ERR_CAND_OVERFLOW = 1, ERR_POOL_OVERFLOW = 2, ERR_QUAD_OVERFLOW = 4, ERR_TRACE_OVERRUN = 8, ERR_CROP_OVERFLOW = 16,
       ERR_TILE_OVERFLOW = 32,
       ERR_TICKET_RUNAWAY = 64,     // a work-queue loop ran more iterations than its list can account for (control flow broken)
       ERR_MARKER_OVERFLOW = 128 }; // more than Workspace::maxm markers in one frame

struct TileDesc { int roi, x0, y0; };   // binarise work unit of the crop pass: x0 = strip index, y0 = first row

struct SquareRec {   // decode's record of one square, slot [frame][quad]; its codes and matches live beside it (Workspace)
    float square[8];    // the square's corners before any orient 2/4 rotation (a candidate's are shift_square of these)
    float patPoint[8];  // the crop quad
    int n_match;        // -1: no quad in the crop (no candidates), else the number of matches in sq_match
    int pad;
};

// counters block (device ints), zeroed at the start of every batch
enum { CNT_FRAME_CANDS = 0, CNT_CROP_ROIS = 1, CNT_CROP_TILES = 2, CNT_CROP_CANDS = 3,
       CNT_POOL_INTS = 4 /* 64-bit, uses 4..5 */, CNT_CROP_QUADS = 6, CNT_TICKET_F = 7, CNT_TICKET_C = 8, CNT_ERR = 9,
       CNT_CROP_PIXELS = 10 /* 64-bit, uses 10..11 */, CNT_LONG_F = 12, CNT_LONG_C = 13, CNT_TICKET_LF = 14, CNT_TICKET_LC = 15,
       CNT_MID_F = 16, CNT_MID_C = 17, CNT_TICKET_MF = 18, CNT_TICKET_MC = 19, CNT_TICKET_BC = 20, CNT_MID_C_FIRST = 21, CNT_TICKET_MC2 = 22,
       CNT_POSE_JOBS = 23,
       CNT_PROF = 24 /* 32 64-bit profiling slots, written only by builds with -DOCVAR_PROF (tools/prof_tier2.py) */,
       CNT_CROP_EARLY = 88, CNT_CROP_REST = 89, CNT_CROP_LIVE = 90 /* entries of the crop pass's lists E, R, R' (croplist_core.h) */, CNT_COUNT = 92 };

struct Workspace {
    // limits
    int max_w, max_h, max_batch;
    int maxq;               // frame-pass quads kept per frame (ocvar_hip_create: OCVAR_MAX_QUADS; ocvar_hip_create_ex/_dense: caller's choice)
    int maxm;               // marker records per frame: MAXM, or the caller's choice on a dense context (ocvar_hip_create_dense)
    int dense;              // 1: made by ocvar_hip_create_dense -- the per-frame tail runs the scalable kernels (order.hip, decode.hip)
    int track_gw, track_gh; // dense: corner grid of the sparse tracking replay (tail_core.h), cells of TRACK_CELL px over max_w x max_h
    int decode_slices;      // dense: waves of decode_kernel per frame (DECODE_SLICES on the other contexts)
    int order_chunk;        // dense: squares per sorted chunk of the ordering (ORDER_CHUNK, or maxq rounded up to a power of two)
    int cap_frame_cands, cap_crop_cands, cap_crop_rois, cap_crop_tiles, cap_crop_quads;
    long long cap_pool_ints, cap_crop_pixels;
    // per batch geometry
    int W, H, sw, sh, ns, n_frames, n_templates;   // ns: columns of a neighbour plane = sw rounded up to 16
    int n_sizes, n_groups, max_match;        // the library (library_core.h): size classes, groups, most matches per square
    int crop_phases;                         // 2: crop tier 2 in two launches (earliest starts first, then the rest behind exact pruning); 1: one launch (few frames: the shorter chain)
    int crop_steps_cap;                      // most steps a walk of the crop pass gets in tier 2 (plan_core.h; >= mid_steps, which the frames pass keeps)
    int mid_steps, mid_blocks, long_blocks;  // tuning (env OCVAR_MID_STEPS / OCVAR_MID_BLOCKS / OCVAR_LONG_BLOCKS): tier-2 step budget and grid, tier-3 grid
    int max_mid_blocks, max_long_blocks;     // slabs allocated at create (scaled with max_batch)
    int short_blocks, crop_blocks;           // grids of follower tier 1 and of the crop binarise kernel (scaled with the batch)
    int frame_strips, frame_chunks, frame_chunk_rows;  // binarise work decomposition of a frame
    // device buffers
    uint8_t* gray;          // [B][H][gray_pitch(W)]: panels of 256 bytes (hd.h::gray_col)
    uint8_t* nbr_frame;     // [B][sh][sw]
    uint8_t* nbr_crop;      // crop pool
    StartCand* cands_frame;
    StartCand* cands_crop;
    StartCand* mid_frame;   // starts whose border exceeded tier 1's step budget
    StartCand* mid_crop;
    StartCand* mid_first_crop;   // crop starts tier 2 takes first (expected longest walks), counter CNT_MID_C_FIRST, capacity cap_long
    StartCand* crop_early;  // two-phase crop pass, the lists cut from mid_crop (croplist_core.h), capacity cap_long each: E, counter CNT_CROP_EARLY
    StartCand* crop_rest;   // R, counter CNT_CROP_REST
    StartCand* crop_live;   // R', counter CNT_CROP_LIVE
    StartCand* long_frame;  // starts whose border exceeded tier 2's step budget
    StartCand* long_crop;
    int cap_long;
    int* pool;              // points + DP stacks
    int* slab;              // [max_mid_blocks*256][SLAB_STRIDE] private point space of the tier-2 lanes
    int* slab3;             // [max_long_blocks*4][SLAB3_STRIDE] point space of the tier-3 waves
    QuadRec* quads_frame;   // [B][maxq] unordered
    int* n_quads_frame;     // [B]
    float* squares;         // [B][maxq][8] ordered, after tracking
    int* n_squares;         // [B]
    int* crop_of;           // [B][maxq] crop ROI index of square i, or -1
    Roi* rois_crop;
    TileDesc* tiles_crop;
    unsigned long long* crop_pixels;   // = counters + CNT_CROP_PIXELS: running sum of crop plane sizes (pool cursor)
    QuadRec* quads_crop;    // pool
    unsigned long long* best_crop;     // [cap_crop_rois] (start<<32 | quad slot), ~0 = none
    int* ring_frame;        // [B] 1: the frame's own frame border is the rectangle ring_quads_kernel has published (tier 1 drops its start)
    int* ring_crop;         // [cap_crop_rois] the same for a crop
    int* crop_min_rest;     // [cap_crop_rois] smallest start position among a crop's tier-2 starts off the crop's frame (tier 2 walks these first)
    SquareRec* sq_recs;     // [B][maxq]
    long long* sq_codes;    // [B][maxq][n_sizes] the code read for each size class
    int* sq_match;          // [B][maxq][max_match] matched groups (group << 2 | orient - 1), ascending
    MarkerRec* prev;        // [B][maxm]
    int* n_prev;            // [B]
    int* reserve;           // [B][maxm] tracked marker indices
    int* n_reserve;         // [B]
    int* pose_jobs;         // [B][maxm] frame * maxm + slot of every output marker (counter CNT_POSE_JOBS): pose_kernel's work list
    MarkerRec* markers;     // [B][maxm] output
    // dense contexts only (nullptr elsewhere)
    int* sorted_starts;     // [B][maxq] the frame's discovery positions, sorted in chunks of ORDER_CHUNK
    float* sq_tmp;          // [B][maxq][8] squares in sequence order before tracking
    int* trk_cells;         // [B][track_gw * track_gh + 1] corner grid: first entry of each cell
    int* trk_fill;          // [B][track_gw * track_gh] fill cursors of the grid build
    int* trk_items;         // [B][4 maxq] square index of each corner entry
    int* trk_next;          // [B][maxq + 1] "next square still in the list" forest of the replay
    int* surv;              // [B][maxq] finalise: the square's survivor (template << 1 | score), -1: none
    int* src;               // [B][maxm] finalise: source of each output record
    int* n_markers;         // [B]
    TemplateRec* templates; // [MAXT]
    SizeClass* sizes;       // [MAX_SIZE_CLASSES]
    LutEntry* lut;          // [4 * MAXT] per size class, sorted by (code, group)
    int* group_off;         // [MAXT + 1] into group_members
    int* group_members;     // [MAXT]
    CameraRec* camera;
    int* counters;          // [CNT_COUNT]
};

// launchers (each enqueues on `stream`, no synchronisation)
// d_bgr holds frames in `format` (OCVAR_FMT_*); grey_in_place is not launched for OCVAR_FMT_GRAY (nothing to write)
void launch_binarise_frames(const Workspace& ws, const uint8_t* d_bgr, int row_stride, size_t frame_stride, int grey_in_place,
                            int format, hipStream_t stream);
void launch_binarise_crops(const Workspace& ws, hipStream_t stream);
void launch_ring_quads_frames(const Workspace& ws, hipStream_t stream);   // the ROIs' own frame borders without a walk (before tier 1)
void launch_ring_quads_crops(const Workspace& ws, hipStream_t stream);
void launch_follow_frames(const Workspace& ws, hipStream_t stream);
void launch_follow_crops(const Workspace& ws, hipStream_t stream);
void launch_follow_mid_frames(const Workspace& ws, hipStream_t stream);
void launch_follow_mid_crops(const Workspace& ws, hipStream_t stream);   // both phases and the list kernels in front of them
void launch_follow_long_frames(const Workspace& ws, hipStream_t stream);
void launch_follow_long_crops(const Workspace& ws, hipStream_t stream);
void launch_order_and_crops(const Workspace& ws, hipStream_t stream);   // (dense contexts: the sort, replay and crop kernels)
void launch_decode(const Workspace& ws, hipStream_t stream);
// (refine.half_win > 0: refine_corners_kernel between the marker records and the poses, refine.hip)
void launch_finalise(const Workspace& ws, const RefineArgs& refine, hipStream_t stream);
void launch_refine_corners(const Workspace& ws, const RefineArgs& refine, hipStream_t stream);

// A batch's board (ocvar_hip_set_board), passed by value in the launch arguments: n entries (0: off) and the context's device
// table -- entries [OCVAR_MAX_BOARD_MARKERS], templateId -> board index map [MAXT] (-1: not on the board), poses [max_batch].
struct BoardArgs {
    int n;
    const BoardEntry* entries;
    const int* map;
    BoardPose* poses;
};
// (board.n > 0: board_pose_kernel, one wave per frame, after launch_finalise; board.hip)
void launch_board_poses(const Workspace& ws, const BoardArgs& board, hipStream_t stream);

// A context's overlays and drawing workspace (ocvar_hip_set_overlay allocates them): the device table, and per record slot of a
// chunk of frames its OverlayDraw and OverlayBox, [max_batch][maxm].
struct OverlayArgs {
    const OverlayTable* table;
    OverlayDraw* draws;
    OverlayBox* boxes;
};
// overlay_setup_kernel + overlay_draw_kernel (overlay.hip) on n_frames frames in `format` and their records recs [n_frames][stride]
// (the first min(counts[f], stride) of frame f), all in device memory
void launch_overlay(const OverlayArgs& oa, uint8_t* frames, int W, int H, long long row_stride, long long frame_stride, int n_frames,
                    int format, const MarkerRec* recs, const int* counts, int stride, hipStream_t stream);

// A context's annotation workspace (the first annotate call allocates it): per record slot of a chunk of frames its AnnoRec and
// AnnoBox, [max_batch][maxm].
struct AnnoArgs {
    AnnoRec* recs;
    AnnoBox* boxes;
};
// annotate_setup_kernel + annotate_draw_kernel (annotate.hip) on n_frames frames in `format` and their records recs
// [n_frames][stride] (the first min(counts[f], stride) of frame f), all in device memory; style and camera by value
void launch_annotate(const AnnoArgs& aa, uint8_t* frames, int W, int H, long long row_stride, long long frame_stride, int n_frames, int format,
                     const MarkerRec* recs, const int* counts, int stride, const OcvarAnnotateStyle& st, const CameraRec& cam,
                     hipStream_t stream);

// One launch of patch_kernel (patch.hip), all pointers in device memory: frames of W x H pixels; of frame f the records
// recs[f * rec_stride + k], k < min(counts[f], slots); patches [n_frames][slots][ph][pw][bpp] at any address; status
// [n_frames][slots] or nullptr; flags OCVAR_PATCH_*.
struct PatchArgs {
    const uint8_t* frames;
    int W, H;
    long long row_stride, frame_stride;
    const MarkerRec* recs;
    const int* counts;
    int rec_stride;
    uint8_t* patches;
    int pw, ph, slots, flags;
    int* status;
};
// n_frames (at most 32768: the grid's z) frames in `format`
void launch_patches(const PatchArgs& a, int n_frames, int format, hipStream_t stream);

// One launch of undistort_kernel (undistort.hip), all pointers in device memory: n_frames frames of W x H pixels from src to dst
// (which do not overlap), rows and frames the given bytes apart, under the camera `cam` (by value: the context's at the call).
struct UndistortArgs {
    const uint8_t* src;
    uint8_t* dst;
    int W, H;
    long long src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride;
    UndistortCam cam;
};
// n_frames (at most 65535: the grid's z) frames in `format`
void launch_undistort(const UndistortArgs& a, int n_frames, int format, hipStream_t stream);

// One launch of undistort_records_kernel: of frame f the records in[f * slots + k], k < min(counts[f], slots), to the same slots
// of out (which may be in).
struct UndistortRecArgs {
    const MarkerRec* in;
    MarkerRec* out;
    const int* counts;
    int slots;
    UndistortCam cam;
};
// n_frames (at most 65535: the grid's y) frames
void launch_undistort_records(const UndistortRecArgs& a, int n_frames, hipStream_t stream);

// One launch of yuv_to_frames_kernel (to_frames) or frames_to_yuv_kernel (yuv.hip) on the n_frames (at most YUV_CHUNK_FRAMES: the
// grid's z) frames of a (yuv_core.h: YuvArgs), whose two sides do not overlap.
constexpr int YUV_CHUNK_FRAMES = 65535;
void launch_yuv(const YuvArgs& a, int n_frames, bool to_frames, hipStream_t stream);
// The same of yuv_ex_to_frames_kernel or yuv_ex_from_frames_kernel (yuv_ex.hip) on the frames of a (yuv_ex_core.h: YuvExArgs).
void launch_yuv_ex(const YuvExArgs& a, int n_frames, bool to_frames, hipStream_t stream);

// One launch of a resize kernel (resize.hip) on the n_frames (at most RESIZE_CHUNK_FRAMES: the grid's z) frames in `format` of a
// (resize_core.h: ResizeArgs), whose two sides do not overlap.
constexpr int RESIZE_CHUNK_FRAMES = 65535;
void launch_resize(const ResizeArgs& a, int n_frames, int format, hipStream_t stream);

// One launch of scale_records_kernel: of frame f the records in[f * slots + k], k < min(counts[f], slots), to the same slots of out
// (which may be in), their squares carried from a sw x sh frame to a dw x dh one; flags OCVAR_SCALE_*, cam by value: the
// context's at the call.
struct ScaleRecArgs {
    const MarkerRec* in;
    MarkerRec* out;
    const int* counts;
    int slots, sw, sh, dw, dh, flags;
    CameraRec cam;
};
// n_frames (at most 65535: the grid's y) frames
void launch_scale_records(const ScaleRecArgs& a, int n_frames, hipStream_t stream);

// One launch of an orient kernel (orient.hip) on the n_frames (at most ORIENT_CHUNK_FRAMES: the grid's z) frames in `format` of a
// (orient_core.h: OrientArgs), whose two sides do not overlap.
constexpr int ORIENT_CHUNK_FRAMES = 65535;
void launch_orient(const OrientArgs& a, int n_frames, int format, hipStream_t stream);

// One launch of orient_records_kernel: of frame f the records in[f * slots + k], k < min(counts[f], slots), to the same slots of out
// (which may be in), their squares carried from a sw x sh frame to its orientation; flags OCVAR_ORIENT_*, cam by value: the
// context's at the call.
struct OrientRecArgs {
    const MarkerRec* in;
    MarkerRec* out;
    const int* counts;
    int slots, sw, sh, orientation, flags;
    CameraRec cam;
};
// n_frames (at most 65535: the grid's y) frames
void launch_orient_records(const OrientRecArgs& a, int n_frames, hipStream_t stream);

// One launch of warp_kernel (warp.hip) on the n_frames (at most WARP_CHUNK_FRAMES: the grid's z) frames in `format` of a
// (warp_core.h: WarpArgs), whose two sides do not overlap.
constexpr int WARP_CHUNK_FRAMES = 65535;
void launch_warp(const WarpArgs& a, int n_frames, int format, hipStream_t stream);

// One launch of warp_records_kernel: of frame f the records in[f * slots + k], k < min(counts[f], slots), to the same slots of out
// (which may be in), their squares carried through the forward map maps[9 f ..] (maps[0 ..] with OCVAR_WARP_ONE_MAP), device
// memory; flags OCVAR_WARP_*, cam by value: the context's at the call.
struct WarpRecArgs {
    const MarkerRec* in;
    MarkerRec* out;
    const int* counts;
    int slots;
    const double* maps;
    int flags;
    CameraRec cam;
};
// n_frames (at most 65535: the grid's y) frames
void launch_warp_records(const WarpRecArgs& a, int n_frames, hipStream_t stream);

// One launch of warp_board_maps_kernel: maps[9 f ..] = warp_board_plane_map(poses[f], K, rect, dw, dh) for f < n_frames; K and rect
// by value.
struct WarpBoardMapArgs {
    const OcvarBoardPose* poses;
    double* maps;
    int n_frames, dw, dh;
    double K[9], rect[4];
};
void launch_warp_board_maps(const WarpBoardMapArgs& a, hipStream_t stream);

// One round of the three levels kernels (levels.hip) on the n_frames (at most LEVELS_WS_FRAMES: the workspace's) frames in
// `format` of a (levels_core.h: LevelsArgs), whose two sides do not overlap: histograms into a.hist, which must be all zeros and is
// all zeros again afterwards (the LUT kernel clears what it has read), LUTs into a.luts, the blend into a.dst.
void launch_levels(const LevelsArgs& a, int n_frames, int format, hipStream_t stream);

// One launch of bayer_to_frames_kernel (bayer.hip) on the n_frames (at most BAYER_CHUNK_FRAMES: the grid's z) mosaics of a
// (bayer_core.h: BayerArgs), whose two sides do not overlap.
constexpr int BAYER_CHUNK_FRAMES = 65535;
void launch_bayer(const BayerArgs& a, int n_frames, hipStream_t stream);

// The pyramids of n_frames frames in `format` (flow.hip: flow_grey_kernel, then flow_down_kernel level by level): frame f's
// levels 0 .. g.L go to pyr + f * slot_bytes, laid out as g says.
struct FlowPyrArgs {
    const uint8_t* frames;
    long long row_stride, frame_stride;
    uint8_t* pyr;
    long long slot_bytes;
    FlowGeom g;
};
// n_frames (at most 65535: the grid's z) frames
void launch_flow_pyramids(const FlowPyrArgs& a, int n_frames, int format, hipStream_t stream);

// One launch of flow_track_kernel: of frame f the records in[f * slots + k], k < min(counts[f], slots), from the pyramid at
// pyr_a + f * slot_bytes to the one at pyr_b + f * slot_bytes, into the same slots of out (which may be in); status
// [n_frames][slots] and err [n_frames][slots][4] or nullptr.  Parameters and camera by value.
struct FlowTrackArgs {
    const uint8_t* pyr_a;
    const uint8_t* pyr_b;
    long long slot_bytes;
    FlowGeom g;
    FlowArgs fa;
    CameraRec cam;
    const MarkerRec* in;
    const int* counts;
    MarkerRec* out;
    int* status;
    float* err;
    int slots, n_frames;
};
void launch_flow_track(const FlowTrackArgs& a, hipStream_t stream);

}  // namespace ocvar
