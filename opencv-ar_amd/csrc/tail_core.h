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
