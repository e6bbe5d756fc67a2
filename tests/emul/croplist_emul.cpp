// croplist_emul.cpp -- host build of the crop pass's list rules and step budget (opencv-ar_amd/csrc/croplist_core.h) and of
// the plan's crop_steps_cap (plan_core.h) for tests/test_crop_lists_cpu.py.  TEST ONLY: nothing in the product links this.
//
// The list emulation follows follow.hip::crop_lists: `waves` waves of 64 lanes stride over the source list in chunks of
// 512 entries, a lane per entry; each wave stages what a target list keeps and appends it once per chunk.  (Waves run one after
// the other here, so a list comes out in one of the orders the device may produce; the tests compare lists as multisets.)
typedef struct ihipStream_t* hipStream_t;   // (kernels.h declares the launchers; nothing here calls one)
#include "plan_core.h"

using namespace ocvar;

namespace {
constexpr int CHUNK = 512;

// prune == 0: src -> out0 (E) and out1 (R) by crop_min_rest; prune != 0: src -> out0 (R') by best_crop
void lists(const StartCand* src, int n, const int* crop_min_rest, const unsigned long long* best_crop, int prune, int waves,
           StartCand* out0, int* n0_out, StartCand* out1, int* n1_out) {
    int c0 = 0, c1 = 0;   // the lists' counters
    for (int wave = 0; wave < waves; wave++)
        for (int base = wave * CHUNK; base < n; base += waves * CHUNK) {
            StartCand stage[2][CHUNK];
            int n0 = 0, n1 = 0;
            const int end = base + CHUNK < n ? base + CHUNK : n;
            for (int i0 = base; i0 < end; i0 += 64)
                for (int lane = 0; lane < 64 && i0 + lane < end; lane++) {
                    const StartCand c = src[i0 + lane];
                    bool to0, to1 = false;
                    if (prune) {
                        to0 = !crop_start_beaten(c.pos, best_crop[c.roi]);
                    } else {
                        to0 = crop_start_earliest(c.pos, crop_min_rest[c.roi]);
                        to1 = !to0;
                    }
                    if (to0) stage[0][n0++] = c;
                    if (to1) stage[1][n1++] = c;
                }
            for (int k = 0; k < n0; k++) out0[c0 + k] = stage[0][k];
            c0 += n0;
            for (int k = 0; k < n1; k++) out1[c1 + k] = stage[1][k];
            c1 += n1;
        }
    *n0_out = c0;
    if (n1_out) *n1_out = c1;
}
}  // namespace

// lists are [n][3] ints (roi, pos, is_hole); every output has room for n entries
extern "C" void croplist_emul_split(const int* src, int n, const int* crop_min_rest, int waves, int* e, int* n_e, int* r, int* n_r) {
    static_assert(sizeof(StartCand) == 3 * sizeof(int), "a list entry is three ints");
    lists(reinterpret_cast<const StartCand*>(src), n, crop_min_rest, nullptr, 0, waves, reinterpret_cast<StartCand*>(e), n_e,
          reinterpret_cast<StartCand*>(r), n_r);
}
extern "C" void croplist_emul_prune(const int* src, int n, const unsigned long long* best_crop, int waves, int* live, int* n_live) {
    lists(reinterpret_cast<const StartCand*>(src), n, nullptr, best_crop, 1, waves, reinterpret_cast<StartCand*>(live), n_live, nullptr,
          nullptr);
}
extern "C" int croplist_emul_budget(int sw, int sh, int mid_steps, int cap) { return crop_walk_budget(sw, sh, mid_steps, cap); }
extern "C" int croplist_emul_no_start() { return CROP_NO_START; }

// out: mid_steps, crop_steps_cap, crop_phases of the batch's plan; knob_set / knob_value as in plan_emul.cpp (6 entries in the
// order of PlanOverrides, or null)
extern "C" void croplist_emul_plan(int width, int height, int n_frames, int max_batch, int gated, const int* knob_set,
                                   const long long* knob_value, int* out) {
    Workspace w{};
    plan_workspace(&w, width, height, max_batch, OCVAR_MAX_QUADS, OCVAR_MAX_MARKERS, false);
    PlanKnob k[6] = {};
    for (int i = 0; i < 6 && knob_set; i++) k[i] = PlanKnob{knob_set[i] != 0, knob_value[i]};
    plan_batch(&w, width, height, n_frames, gated != 0, PlanOverrides{k[0], k[1], k[2], k[3], k[4], k[5]});
    out[0] = w.mid_steps;
    out[1] = w.crop_steps_cap;
    out[2] = w.crop_phases;
}
