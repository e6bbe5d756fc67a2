// plan_emul.cpp -- host build of the workspace sizing and the batch plan (opencv-ar_amd/csrc/plan_core.h) for
// tests/test_batch_plan_cpu.py.  TEST ONLY: nothing in the product links this.
typedef struct ihipStream_t* hipStream_t;   // (kernels.h declares the launchers; nothing here calls one)
#include "plan_core.h"

using namespace ocvar;

// the fields the plan decides, as the test reads them
struct PlanOut {
    long long cap_pool_ints, cap_crop_pixels;
    int cap_frame_cands, cap_crop_cands, cap_crop_rois, cap_crop_tiles, cap_crop_quads, cap_long;
    int max_mid_blocks, max_long_blocks, track_gw, track_gh, decode_slices, order_chunk;
    int W, H, sw, sh, ns, n_frames;
    int frame_strips, frame_chunk_rows, frame_chunks, mid_steps, crop_phases, mid_blocks, long_blocks, short_blocks, crop_blocks;
};

// knob_set / knob_value: 6 entries in the order of PlanOverrides, or null for no overrides
extern "C" void plan_emul(int max_w, int max_h, int max_batch, int max_quads, int max_markers, int dense, int width, int height,
                          int n_frames, int gated, const int* knob_set, const long long* knob_value, PlanOut* o) {
    Workspace w{};
    plan_workspace(&w, max_w, max_h, max_batch, max_quads, max_markers, dense != 0);
    PlanKnob k[6] = {};
    for (int i = 0; i < 6 && knob_set; i++) k[i] = PlanKnob{knob_set[i] != 0, knob_value[i]};
    plan_batch(&w, width, height, n_frames, gated != 0, PlanOverrides{k[0], k[1], k[2], k[3], k[4], k[5]});
    *o = PlanOut{w.cap_pool_ints, w.cap_crop_pixels, w.cap_frame_cands, w.cap_crop_cands, w.cap_crop_rois, w.cap_crop_tiles,
                 w.cap_crop_quads, w.cap_long, w.max_mid_blocks, w.max_long_blocks, w.track_gw, w.track_gh, w.decode_slices,
                 w.order_chunk, w.W, w.H, w.sw, w.sh, w.ns, w.n_frames, w.frame_strips, w.frame_chunk_rows, w.frame_chunks,
                 w.mid_steps, w.crop_phases, w.mid_blocks, w.long_blocks, w.short_blocks, w.crop_blocks};
}
extern "C" int plan_emul_march_strip() { return MARCH_STRIP; }
extern "C" int plan_emul_tile_rows() { return NBR_TILE_H; }
