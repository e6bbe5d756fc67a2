// tail_core.h -- per-frame sequential tail of cvarArMultRegistration: tracking association and the greedy
// candidate elimination.  Both are order-dependent by definition in the reference, so one lane per frame
// replays them verbatim on the device (frames are independent, so a batch still fills the chip).
//
// Replaces /root/reference/src/opencvar.cpp:592-617 (cvarTrack), 635-668 (tracking loop with its
// erase-while-iterating behaviour), 780-792 (|| dedupe) and 795-801 (output selection).
#pragma once
#include "hd.h"
#include "library_core.h"
#include <math.h>

namespace ocvar {

struct MarkerRec {  // == CvarMarker (include/opencvar/opencvar.h), 184 bytes
    double glMatrix[16];
    int templateId;
    int markerId;
    double score;
    float square[8];
    double aspectRatio;
};

// cvarTrack: all four corners within 20 px under one cyclic shift; on success pt1 takes pt2's corners.
OCVAR_HD int track_square(float* pt1, const float* pt2) {
    for (int j = 0; j < 4; j++) {
        int res = 0;
        for (int i = 0; i < 4; i++) {
            const int k = (i + j) & 3;
            const double dx = (double)pt1[2 * i] - (double)pt2[2 * k], dy = (double)pt1[2 * i + 1] - (double)pt2[2 * k + 1];
            if (sqrt(dx * dx + dy * dy) < 20) res++;
        }
        if (res == 4) {
            float t[8];
            for (int i = 0; i < 4; i++) {
                const int k = (i + j) & 3;
                t[2 * i] = pt2[2 * k];
                t[2 * i + 1] = pt2[2 * k + 1];
            }
            for (int i = 0; i < 8; i++) pt1[i] = t[i];
            return 1;
        }
    }
    return 0;
}

// Tracking loop: squares (n quads of 4 float points, list order) is compacted in place exactly as
// vector::erase does; reserve receives marker indices (duplicates possible).  Returns the new quad count.
OCVAR_HD int track_markers(MarkerRec* markers, int n_markers, float* squares, int n_quads, int* reserve, int max_reserve,
                           int* n_reserve) {
    int nr = 0;
    for (int i = 0; i < n_markers; i++) {
        for (int j = 0; j < n_quads; j++) {
            if (track_square(markers[i].square, squares + 8 * j)) {
                if (nr < max_reserve) reserve[nr] = i;
                nr++;
                for (int k = 8 * j; k < 8 * (n_quads - 1); k++) squares[k] = squares[k + 8];
                n_quads--;
                // the reference's loop index is not corrected after the erase: the next quad is skipped
            }
        }
    }
    *n_reserve = nr;
    return n_quads;
}

// ---- the tracking loop in sparse form (dense contexts: up to 4096 markers x 16384 squares per frame) ----
// Same result as track_markers, bit for bit, without its O(markers x squares) scan and O(squares) shift per match.
// track_square(m, q) can only succeed when m's corner 0 lies within 20 px of a corner of q (|dx|, |dy| < 20), so the squares a
// marker can take are found in the 3 x 3 cells of TRACK_CELL px around its corner 0 in a grid of all squares' corners.  The
// loop's order rules, restated on the ORIGINAL list indices of the squares:
//   - marker i examines the squares still in the list in list order; the first one it matches is the lowest index >= pos that
//     matches with its current corners (a failed track_square changes nothing), wherever it lies in the grid;
//   - a match erases that square and the loop index is not corrected: the next square still in the list is skipped, the marker
//     goes on behind it (pos = that square + 1), with its updated corners.
// Erased squares are skipped with a "next square still in the list" forest (next[i] == i: i is in the list; erasing i sets
// next[i] = i + 1; path halving).  The caller compacts the list afterwards (next[i] == i, in index order).
constexpr int TRACK_CELL = 32;   // >= 20: a point within 20 px of another lies in the same or a neighbouring cell

// grid cell of one coordinate, clamped to [0, n) -- monotone and 1-Lipschitz in cells, so the 3 x 3 rule survives clamping
// (negative and NaN coordinates go to cell 0: a NaN corner never matches anyway)
OCVAR_HD int track_cell(float v, int n) {
    if (!(v >= 0.f)) return 0;
    const float c = v / (float)TRACK_CELL;   // (exact: a power of two)
    if (c >= (float)(n - 1)) return n - 1;
    return (int)c;
}

// cells of a grid covering [0, w) x [0, h) px
OCVAR_HD int track_grid_cells(int w, int h, int* gw, int* gh) {
    *gw = (w + TRACK_CELL - 1) / TRACK_CELL > 0 ? (w + TRACK_CELL - 1) / TRACK_CELL : 1;
    *gh = (h + TRACK_CELL - 1) / TRACK_CELL > 0 ? (h + TRACK_CELL - 1) / TRACK_CELL : 1;
    return *gw * *gh;
}

// The grid by counting sort, sequentially: cell_start [gw*gh + 1], items [4 n] (one entry per corner; a square can appear
// more than once in a neighbourhood).  The device builds the same lists in parallel, in another order within a cell: the
// replay takes the lowest matching index, so it does not depend on that order.
OCVAR_HD void track_grid_build(const float* squares, int n, int gw, int gh, int* cell_start, int* items) {
    const int nc = gw * gh;
    for (int c = 0; c <= nc; c++) cell_start[c] = 0;
    for (int j = 0; j < 4 * n; j++) cell_start[track_cell(squares[2 * j + 1], gh) * gw + track_cell(squares[2 * j], gw) + 1]++;
    for (int c = 0; c < nc; c++) cell_start[c + 1] += cell_start[c];
    for (int j = 0; j < 4 * n; j++) {
        const int c = track_cell(squares[2 * j + 1], gh) * gw + track_cell(squares[2 * j], gw);
        items[cell_start[c]++] = j >> 2;
    }
    for (int c = nc; c > 0; c--) cell_start[c] = cell_start[c - 1];
    cell_start[0] = 0;
}

OCVAR_HD int track_next_alive(int* next, int i) {
    while (next[i] != i) {
        next[i] = next[next[i]];
        i = next[i];
    }
    return i;
}

// would track_square(m, q) succeed? (m unchanged)
OCVAR_HD bool track_test(const float* m, const float* q) {
    float t[8];
    for (int k = 0; k < 8; k++) t[k] = m[k];
    return track_square(t, q) != 0;
}

// The lowest square index >= pos still in the list that marker corners m match (n: none).
OCVAR_HD int track_first_match(const float* m, const float* squares, int n, int pos, const int* cell_start, const int* items, int gw,
                               int gh, const int* next) {
    const int cx = track_cell(m[0], gw), cy = track_cell(m[1], gh);
    int best = n;
    for (int y = cy > 0 ? cy - 1 : 0; y <= cy + 1 && y < gh; y++)
        for (int x = cx > 0 ? cx - 1 : 0; x <= cx + 1 && x < gw; x++)
            for (int e = cell_start[y * gw + x]; e < cell_start[y * gw + x + 1]; e++) {
                const int j = items[e];
                if (j >= pos && j < best && next[j] == j && track_test(m, squares + 8 * j)) best = j;
            }
    return best;
}

// One frame: squares [n][8] (read only), next [n + 1] (scratch, set here), the grid of track_grid_build.  Returns the number
// of squares left in the list (those with next[i] == i, i < n).
OCVAR_HD int track_markers_sparse(MarkerRec* markers, int n_markers, const float* squares, int n_quads, const int* cell_start,
                                  const int* items, int gw, int gh, int* next, int* reserve, int max_reserve, int* n_reserve) {
    for (int j = 0; j <= n_quads; j++) next[j] = j;
    int nr = 0, left = n_quads;
    for (int i = 0; i < n_markers; i++) {
        int pos = 0;
        for (;;) {
            const int j = track_first_match(markers[i].square, squares, n_quads, pos, cell_start, items, gw, gh, next);
            if (j >= n_quads) break;
            track_square(markers[i].square, squares + 8 * j);
            if (nr < max_reserve) reserve[nr] = i;
            nr++;
            next[j] = j + 1;
            left--;
            const int skipped = track_next_alive(next, j + 1);
            if (skipped >= n_quads) break;
            pos = skipped + 1;
        }
    }
    *n_reserve = nr;
    return left;
}

// The order of cvarFindSquares (opencvar.cpp:187-214): square i of a frame goes to slot "number of squares with a larger
// discovery position".  Dense contexts count it with binary searches in sorted chunks of the frame's starts (sorted: one
// chunk of starts in ascending order, len of them): squares of the chunk whose start is larger than `start`.
constexpr int ORDER_CHUNK = 2048;   // starts sorted per workgroup in LDS (order.hip: order_sort_kernel), a power of two

// One compare-exchange of the bitonic network that sorts a chunk ascending (stage k = 2, 4, .. len, step j = k / 2, .. 1; len / 2
// threads tid, each one pair per step).
OCVAR_HD void bitonic_step(int* key, int k, int j, int tid) {
    const int i = 2 * tid - (tid & (j - 1)), p = i + j;   // pair (i, i + j), bit j of i clear
    const int a = key[i], b = key[p];
    if ((a > b) == ((i & k) == 0)) {
        key[i] = b;
        key[p] = a;
    }
}

OCVAR_HD int count_greater_sorted(const int* sorted, int len, int start) {
    int lo = 0, hi = len;   // first element > start
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] > start) hi = mid;
        else lo = mid + 1;
    }
    return len - lo;
}

// Greedy elimination (opencvar.cpp:780-792): markerId[i] = -1 marks a loser.
OCVAR_HD void dedupe(int* markerId, const int* templateId, const double* score, int n) {
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++)
            if (markerId[i] == markerId[j] || templateId[i] == templateId[j]) {
                if (score[i] > score[j])
                    markerId[j] = -1;
                else
                    markerId[i] = -1;
            }
}

// The survivors of dedupe without its candidate list.  In the reference every valid square (one whose crop has a quad) holds all
// K templates in order, score 1 where the code matched; a score-1 candidate never loses to a later one, and a score-0 candidate
// outside the first valid square loses on arrival (an earlier square holds its template).  So the survivors are, in candidate
// order:
//   the first valid square: its first score-1 template, else template 0 with score 0 -- unless a later square matches
//   template 0;
//   every later square: the lowest template it matches that no earlier square matched.
// Templates of one group match together, so "no earlier square matched" is a property of the group: earliest[g] is the first
// square that matches group g (NO_SQUARE: none), and a square's survivor is the first member of its lowest group g with
// earliest[g] == itself (groups are numbered in the order of their first members).  tests/test_template_library_cpu.py checks
// this against dedupe on every score pattern of up to 4 squares x 4 templates.
constexpr int NO_SQUARE = 0x7fffffff;

// Survivor of valid square i (first: i is the frame's first valid square) with matches m[0..n): its template, or -1.
OCVAR_HD int square_survivor(int i, bool first, int n, const int* m, const int* earliest, const int* group_off, const int* members,
                             int* score) {
    int best = NO_SQUARE;
    for (int k = 0; k < n; k++) {
        const int g = match_group(m[k]);
        if (earliest[g] == i && g < best) best = g;
    }
    if (best != NO_SQUARE) {
        *score = 1;
        return members[group_off[best]];
    }
    *score = 0;
    return first && n == 0 && earliest[0] == NO_SQUARE ? 0 : -1;   // (template 0 is the first member of group 0)
}

// One frame, sequentially: n_match[i] < 0 marks a square without a crop quad; square i's matches are match[i * stride ..].
// earliest: scratch of n_groups ints.  Writes up to max_out survivors (square, template, score) and returns their number.
OCVAR_HD int sparse_dedupe(int n_sq, const int* n_match, const int* match, int stride, int n_groups, const int* group_off,
                           const int* members, int* earliest, int* out_sq, int* out_t, int* out_score, int max_out) {
    for (int g = 0; g < n_groups; g++) earliest[g] = NO_SQUARE;
    for (int i = n_sq - 1; i >= 0; i--)
        for (int k = 0; k < n_match[i]; k++) earliest[match_group(match[(long long)i * stride + k])] = i;
    int n = 0;
    bool first = true;
    for (int i = 0; i < n_sq; i++) {
        if (n_match[i] < 0) continue;
        int score;
        const int t = square_survivor(i, first, n_match[i], match + (long long)i * stride, earliest, group_off, members, &score);
        first = false;
        if (t < 0) continue;
        if (n < max_out) {
            out_sq[n] = i;
            out_t[n] = t;
            out_score[n] = score;
        }
        n++;
    }
    return n;
}

}  // namespace ocvar
