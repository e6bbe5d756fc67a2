// library_emul.cpp -- host build of the template-library cores (opencv-ar_amd/csrc/library_core.h, the sparse elimination of
// tail_core.h) for tests/test_template_library_cpu.py.  TEST ONLY: nothing in the product links this.
#include "tail_core.h"
#include <cstring>
#include <vector>

using namespace ocvar;

static Library g_lib;

// Builds the table of n templates; -1: more size classes than the library takes.
extern "C" int lib_set(const TemplateRec* t, int n) { return build_library(t, n, &g_lib) ? 0 : -1; }
// n_sizes, n_groups, max_match
extern "C" void lib_info(int* out) {
    out[0] = (int)g_lib.sizes.size();
    out[1] = g_lib.n_groups();
    out[2] = g_lib.max_match;
}
extern "C" void lib_size(int s, int* wh) {
    wh[0] = g_lib.sizes[s].width;
    wh[1] = g_lib.sizes[s].height;
}
extern "C" void lib_groups(int* group_of, int* size_of, int* group_off, int* members) {
    const size_t n = g_lib.group_of.size();
    std::memcpy(group_of, g_lib.group_of.data(), n * sizeof(int));
    std::memcpy(size_of, g_lib.size_of.data(), n * sizeof(int));
    std::memcpy(group_off, g_lib.group_off.data(), g_lib.group_off.size() * sizeof(int));
    std::memcpy(members, g_lib.members.data(), n * sizeof(int));
}

// What decode does with a square's codes (one per size class): the runs of the size classes' tables merged into the square's
// match list.  Returns its length.
extern "C" int lib_square_matches(const long long* codes, int* matches) {
    int n = 0;
    for (size_t s = 0; s < g_lib.sizes.size(); s++) {
        int cnt;
        const int lo = lut_find(g_lib.lut.data(), g_lib.sizes[s].lut_begin, g_lib.sizes[s].lut_count, codes[s], &cnt);
        for (int e = lo; e < lo + cnt; e++) n = insert_match(matches, n, g_lib.lut[e].group << 2 | (g_lib.lut[e].orient - 1));
    }
    return n;
}

// Candidate t's corners from the square's match list (prefix_shift + shift_square).
extern "C" void lib_candidate_square(const float* sq, const int* matches, int n, int t, float* out) {
    shift_square(sq, prefix_shift(matches, n, g_lib.group_off.data(), g_lib.members.data(), t), out);
}

// The reference's way: match_orient for every template in order, rot_square on orient 4 / 2, corners after each (K x 8 floats).
extern "C" void linear_candidates(const TemplateRec* t, int n, const long long* code_of_template, const float* sq, int* orient,
                                  float* squares) {
    float pts[8];
    std::memcpy(pts, sq, sizeof pts);
    for (int j = 0; j < n; j++) {
        orient[j] = match_orient(code_of_template[j], t[j]);
        if (orient[j] == 4) rot_square(pts, 2);
        else if (orient[j] == 2) rot_square(pts, 4);
        std::memcpy(squares + 8 * j, pts, sizeof pts);
    }
}

// Sparse survivors (sparse_dedupe) against the literal loop (dedupe) on one frame: n_match[i] < 0 marks a square without a crop
// quad, the others hold all K templates, score 1 where the template's group is among the square's matches.  Returns 1 when
// both give the same survivors (square, template, score) in the same order; n_out[0], n_out[1]: survivors of each.
extern "C" int dedupe_agrees(int n_sq, int K, const int* n_match, const int* match, int stride, int n_groups, const int* group_of,
                             const int* group_off, const int* members, int* n_out) {
    std::vector<int> mid, tid;
    std::vector<double> score;
    std::vector<char> hit(n_groups);
    for (int i = 0; i < n_sq; i++) {
        if (n_match[i] < 0) continue;
        std::fill(hit.begin(), hit.end(), 0);
        for (int k = 0; k < n_match[i]; k++) hit[match_group(match[(size_t)i * stride + k])] = 1;
        for (int t = 0; t < K; t++) {
            mid.push_back(i);
            tid.push_back(t);
            score.push_back(hit[group_of[t]] ? 1.0 : 0.0);
        }
    }
    const std::vector<int> mid0 = mid;
    dedupe(mid.data(), tid.data(), score.data(), (int)mid.size());
    std::vector<int> lit_sq, lit_t, lit_s;
    for (size_t a = 0; a < mid.size(); a++)
        if (mid[a] >= 0) {
            lit_sq.push_back(mid0[a]);
            lit_t.push_back(tid[a]);
            lit_s.push_back((int)score[a]);
        }
    std::vector<int> earliest(n_groups), sq(n_sq + 1), t(n_sq + 1), s(n_sq + 1);
    const int n = sparse_dedupe(n_sq, n_match, match, stride, n_groups, group_off, members, earliest.data(), sq.data(), t.data(),
                                s.data(), n_sq + 1);
    n_out[0] = (int)lit_sq.size();
    n_out[1] = n;
    if (n != (int)lit_sq.size()) return 0;
    for (int k = 0; k < n; k++)
        if (sq[k] != lit_sq[k] || t[k] != lit_t[k] || s[k] != lit_s[k]) return 0;
    return 1;
}
