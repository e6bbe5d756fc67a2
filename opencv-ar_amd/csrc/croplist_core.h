// croplist_core.h -- which of a crop's tier-2 starts each phase of the crop pass walks, and how many steps a crop's walk
// gets, free of HIP calls: follow.hip's list kernels and hand-out use these, tests/emul/croplist_emul.cpp builds them for the
// host (tests/test_crop_lists_cpu.py).
//
// Of a crop's quads only the one that starts earliest is used, so the crop pass walks in two launches (follow.hip, "Crops:
// exact pruning"): phase 1 the starts on the crops' frames (mid_first_crop) and each crop's earliest other start, phase 2 what
// is left and is not behind its crop's best quad.  Tier 1 writes all starts off the crops' frames to one list, mid_crop; the
// rules below cut it into the lists the phases read:
//   E  (crop_early): the entries phase 1 takes          -- crop_split_kernel, before phase 1
//   R  (crop_rest):  all the others                     -- crop_split_kernel
//   R' (crop_live):  the entries of R not beaten yet    -- crop_prune_kernel, between the phases
#pragma once
#include "hd.h"

namespace ocvar {

constexpr int CROP_NO_START = 0x7fffffff;          // crop_min_rest of a crop that tier 1 routed no start of
constexpr unsigned long long CROP_NO_QUAD = ~0ull; // best_crop of a crop without a quad

// the entry is its crop's earliest start off the crop's frame (crop_min_rest: the smallest pos tier 1 routed for the crop)
OCVAR_HD bool crop_start_earliest(int pos, int crop_min_rest) { return pos == crop_min_rest; }
// the entry starts behind its crop's best quad (best_crop: start << 32 | quad slot): its border can never replace that quad
OCVAR_HD bool crop_start_beaten(int pos, unsigned long long best_crop) { return (unsigned)(best_crop >> 32) < (unsigned)pos; }

// Step budget of one walk in a crop of sw x sh pixels.  A crop's longest border is its own frame border merged with the marker's
// edge where the two touch: on the benchmark's frames at most 1.37 x 4 (sw + sh) steps, so 6 (sw + sh) -- rounded up to whole
// blocks of steps, the unit the budget is checked in -- lets it close in tier 2 instead of being walked again by tier 3.  Never
// below the batch's mid_steps, never above its cap (plan_core.h: crop_steps_cap; equal to mid_steps where the budget is short
// on purpose).
constexpr int CROP_BUDGET_FACTOR = 6, CROP_BUDGET_BLOCK = 32;
OCVAR_HD int crop_walk_budget(int sw, int sh, int mid_steps, int cap) {
    int b = (CROP_BUDGET_FACTOR * (sw + sh) + CROP_BUDGET_BLOCK - 1) & ~(CROP_BUDGET_BLOCK - 1);
    b = b > mid_steps ? b : mid_steps;
    return b < cap ? b : cap;
}

}  // namespace ocvar
