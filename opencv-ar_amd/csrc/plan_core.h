// plan_core.h -- how a context's workspace is sized and how a batch is cut into work, free of HIP calls (api.hip allocates and
// launches by these numbers; tests/emul/plan_emul.cpp builds them for the host, tests/test_batch_plan_cpu.py pins them).
//
// The kernels rely on what is decided here: binarise.hip on frame_chunk_rows being whole tile rows and the chunks covering sh,
// the followers on their grids staying within the slabs allocated for max_mid_blocks / max_long_blocks and on cap_long.
#pragma once
#include "kernels.h"

namespace ocvar {

// A result-invariant launch parameter as api.hip resolved it (the context's ocvar_hip_set_tuning value; profiling builds: else
// the environment's): absent, or a value -- 0 and negative numbers are values.  What a value means, how it is clamped and what
// holds when it is absent is decided below.
struct PlanKnob {
    bool set;
    long long value;
};
inline long long knob_or(PlanKnob k, long long dflt) { return k.set ? k.value : dflt; }

struct PlanOverrides {
    PlanKnob crop_phases, mid_steps, mid_blocks, long_blocks, short_blocks, min_units;   // OCVAR_TUNE_* of the same names
};

inline long long plan_min(long long a, long long b) { return a < b ? a : b; }
inline long long plan_max(long long a, long long b) { return a > b ? a : b; }

// The limits and capacities of a context's workspace (Workspace, "limits" and the slab / list capacities further down): every
// array of the workspace is allocated by these.  The arguments are within what ocvar_hip_create* admits (sides 16 .. 32767,
// max_batch, max_quads, max_markers >= 1).
inline void plan_workspace(Workspace* wp, int max_width, int max_height, int max_batch, int max_quads, int max_markers, bool dense) {
    Workspace& w = *wp;
    w.max_w = max_width;
    w.max_h = max_height;
    w.max_batch = max_batch;
    w.maxq = max_quads;
    w.maxm = max_markers;
    w.dense = dense ? 1 : 0;
    const long long B = max_batch, WH = (long long)max_width * max_height;
    const long long per_frame_cands = WH / 16 < 16384 ? 16384 : WH / 16;
    w.cap_frame_cands = (int)plan_min(B * per_frame_cands, 1ll << 30);
    w.cap_crop_cands = w.cap_frame_cands;
    w.cap_crop_rois = (int)(B * max_quads);
    // (dense contexts: a crop of a marker-sized square is one or two work units; room for four per square)
    w.cap_crop_tiles = (int)plan_min(B * (dense ? plan_max(4096, 4ll * max_quads) : 4096), 1ll << 30);
    w.cap_crop_quads = (int)(B * max_quads * 4);
    // only tier-2 borders with more corner points than a lane slab holds land here; the fixed part lets a small context take
    // a pathological frame (full-frame noise: thousands of long ragged borders)
    w.cap_pool_ints = B * (1 << 18) + (1 << 24);
    // (bytes of the crops' bit planes: a crop's plane is at most half the bytes of its neighbour-mask byte plane, ns x (sh
    // rounded up to 8), which this pool was sized for at 2 B (W + 16) (H + 8) bytes)
    w.cap_crop_pixels = B * (max_width + 16) * (max_height + 8);
    // (a dense grid of squares covers the frame with crops that overlap their neighbours' -- each crop reaches 5 px past its
    // square and rounds up to whole 16 x 14 tiles: room for four times the frame's plane)
    if (dense) w.cap_crop_pixels *= 4;
    // follower grids (and their slabs) scale with the batch: a one-frame context (the reference's per-frame call) does not
    // need -- or pay for -- the 512 + 1024 workgroups that keep a 2048-frame batch busy
    w.max_mid_blocks = (int)plan_min(MID_BLOCKS_MAX, plan_max(32, B));
    w.max_long_blocks = (int)plan_min(LONG_BLOCKS_MAX, plan_max(128, B * 8));
    w.cap_long = (int)plan_min(plan_max(B * 4096, 1ll << 18), 1ll << 28);   // survivors of tier 1 / tier 2: a noise frame has ~10^4
    if (dense) {   // the scalable tail (follow.hip: order_sort .. crops_kernel; decode.hip: finalise_kernel<true>)
        (void)track_grid_cells(max_width, max_height, &w.track_gw, &w.track_gh);
        w.decode_slices = (int)plan_max(4, plan_min(64, max_quads / 64));   // (4: decode.hip DECODE_SLICES)
        for (w.order_chunk = 2; w.order_chunk < max_quads && w.order_chunk < ORDER_CHUNK;) w.order_chunk <<= 1;
    }
}

// The geometry and the grids of one batch of n_frames frames of width x height pixels on the context whose limits w holds
// (plan_workspace); gated: the context shares the GPU with others (it has a gate).  The arguments are within what enqueue
// admits (16 <= width <= max_w, 16 <= height <= max_h, 1 <= n_frames <= max_batch).
inline void plan_batch(Workspace* wp, int width, int height, int n_frames, bool gated, const PlanOverrides& ov) {
    Workspace& w = *wp;
    w.W = width;
    w.H = height;
    w.sw = width & ~1;
    w.sh = height & ~1;
    w.ns = (w.sw + 15) & ~15;
    w.n_frames = n_frames;
    // Tier 2's step budget: a batch of a few frames has too few borders to fill the GPU with one-lane walks, and its
    // duration is then the longest walk (~800 one-microsecond steps around a crop) -- such batches hand everything longer
    // than 128 steps to the wave tier, which crosses straight runs 64 pixels at a time (1080p, one frame per call: 3.2 ->
    // 2.5 ms).  Large batches keep the long budget: there the one-lane walks are what fills the machine.
    w.mid_steps = (int)knob_or(ov.mid_steps, n_frames <= 8 ? 128 : MID_STEPS);
    if (w.mid_steps < 32) w.mid_steps = 32;
    // The crop pass's walks get a budget that fits their crop (croplist_core.h: crop_walk_budget), up to this cap: in a
    // throughput batch the merged frame border of a large quad-less crop (up to ~1900 steps in a 250 px crop) then closes in
    // tier 2 instead of burning mid_steps there and being walked again by a whole wave of tier 3.  Where the budget is short
    // on purpose -- the latency plan above, or a caller's own mid_steps -- the cap equals it: no effect.
    w.crop_steps_cap = (n_frames > 8 && !ov.mid_steps.set) ? (int)plan_max(CROP_STEPS_CAP, w.mid_steps) : w.mid_steps;
    // Crop tier 2 in two phases saves half of its steps but chains two launches: throughput for batches (+1..2 %), 0.1 ms of
    // latency for a one-frame call -- which therefore keeps the single launch.
    w.crop_phases = knob_or(ov.crop_phases, n_frames <= 8 ? 1 : 2) == 1 ? 1 : 2;
    // Tier 2's grid: alone on the GPU a context wants every lane it can get (its duration is a chain of dependent loads; 1024
    // workgroups: 2.8 ms for the crop pass of 2048 frames, 256: 4.6 ms).  A context that shares the GPU with others (it has a
    // gate) takes a quarter: tier 2's 110-register waves then leave room for the other contexts' binarise waves (4 contexts:
    // 171 -> 176 k frames/s; 128 or 512 workgroups: 171 / 173 k).
    w.mid_blocks = (int)knob_or(ov.mid_blocks, gated ? plan_max(32, w.max_mid_blocks / 4) : w.max_mid_blocks);
    if (w.mid_blocks < 1 || w.mid_blocks > w.max_mid_blocks) w.mid_blocks = w.max_mid_blocks;
    w.long_blocks = (int)knob_or(ov.long_blocks, w.max_long_blocks);
    if (w.long_blocks < 1 || w.long_blocks > w.max_long_blocks) w.long_blocks = w.max_long_blocks;
    // the fixed grids of the work-queue kernels shrink with the batch: a one-frame call does not launch (and wait out) the
    // thousands of workgroups that keep a 2048-frame batch busy
    w.short_blocks = (int)knob_or(ov.short_blocks, n_frames >= 128 ? 1024 : (n_frames * 8 < 16 ? 16 : n_frames * 8));
    if (w.short_blocks < 1 || w.short_blocks > 65535) w.short_blocks = 1024;
    w.crop_blocks = n_frames >= 128 ? 2048 : (n_frames * 16 < 32 ? 32 : n_frames * 16);
    w.frame_strips = (w.sw + MARCH_STRIP - 1) / MARCH_STRIP;
    // rows per binarise work unit: even, chunks of equal size.  Every chunk re-reads ~12 halo rows, so chunks are as
    // tall as the batch allows while the launch still has >= 64K waves (OCVAR_TUNE_MIN_UNITS); never < ~128 rows.  (Measured:
    // choosing the count to fill whole "rounds" of resident waves is no better -- the kernel is issue-bound, not round-bound --
    // and three 360-row chunks per 1080p frame were 20 % slower than eight 136-row ones at 256 frames.)
    int chunks = (w.sh + 64) / 128;
    if (chunks < 1) chunks = 1;
    // (a context that shares the GPU -- it has a gate -- takes the tallest chunks that still give 16 K units: at 2048 frames one
    // 1080-row chunk per strip.  Alone that launch is 8 % slower than four 272-row chunks, 5.9 against 5.4 ms -- fewer, longer
    // waves hide less --, with four contexts in flight it is the faster one: 192 against 185 k frames/s, fewer halo rows and
    // fewer workgroup turnovers for the other contexts' kernels to queue behind)
    const long long min_units = knob_or(ov.min_units, gated ? 16384 : 65536);
    while (chunks > 1 && (long long)w.frame_strips * (chunks / 2) * n_frames >= min_units) chunks /= 2;
    int rows = (w.sh + chunks - 1) / chunks;
    rows = (rows + NBR_TILE_H - 1) / NBR_TILE_H * NBR_TILE_H;   // whole tile rows (14) per work unit: binarise.hip writes the bit plane tile by tile
    w.frame_chunk_rows = rows;
    w.frame_chunks = (w.sh + rows - 1) / rows;
}

}  // namespace ocvar
