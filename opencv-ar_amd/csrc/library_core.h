// library_core.h -- the template library as the decode and the elimination see it: size classes, groups, code lookup.
//
// The reference compares every square's read code with every template in turn (cvarArMultRegistration,
// /root/reference/src/opencvar.cpp:700-777), so its work per square grows with the library.  Here the read code depends on the
// template only through its code-grid size (the destination patch is (tw+2) x (th+2)), so a square is read once per distinct size
// -- a SIZE CLASS -- and the read code is looked up in a table sorted by code:
//   group     templates with identical size and code[4]; they match (and orient) together.  Groups are numbered in the order of
//             their first member, so a smaller group number means a smaller first template.
//   LutEntry  (code, group, orient) for each distinct code[k] of a group (k = orient - 1; a rotationally symmetric code keeps
//             its first k, as match_orient does), sorted by (code, group) within each size class.
// build_library runs on the host (ocvar_hip_set_templates); lut_find and the D4 helpers run on both sides.
#pragma once
#include "decode_core.h"

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

namespace ocvar {

constexpr int MAX_SIZE_CLASSES = 16;   // distinct (width, height) code sizes per library (OCVAR_E_ARG above)

struct SizeClass { int width, height, lut_begin, lut_count; };
struct LutEntry { long long code; int group, orient; };

// A square's match: group << 2 | (orient - 1).
OCVAR_HD int match_group(int m) { return m >> 2; }
OCVAR_HD int match_orient_of(int m) { return (m & 3) + 1; }

// First index and count of the entries of lut[begin, begin + count) whose code is `bit` (binary search, then the run).
OCVAR_HD int lut_find(const LutEntry* lut, int begin, int count, long long bit, int* n) {
    int lo = begin, hi = begin + count;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lut[mid].code < bit) lo = mid + 1;
        else hi = mid;
    }
    int e = lo;
    while (e < begin + count && lut[e].code == bit) e++;
    *n = e - lo;
    return lo;
}

// Inserts match m into a square's ascending list out[0..n); returns the new length.
OCVAR_HD int insert_match(int* out, int n, int m) {
    int j = n;
    for (; j > 0 && out[j - 1] > m; j--) out[j] = out[j - 1];
    out[j] = m;
    return n + 1;
}

// The orient 2/4 corner rotation as a cyclic shift of the corners: rot_square(pts, 2) (orient 4) moves corner j to
// j + 1, rot_square(pts, 4) (orient 2) to j + 3; successive rotations add up mod 4.
OCVAR_HD int orient_shift(int orient) { return orient == 4 ? 1 : (orient == 2 ? 3 : 0); }
OCVAR_HD void shift_square(const float* sq, int s, float* out) {
    for (int j = 0; j < 4; j++) {
        const int k = (j - s) & 3;
        out[2 * j] = sq[2 * k];
        out[2 * j + 1] = sq[2 * k + 1];
    }
}

// Members of a group that are <= t (members[off[g] .. off[g+1]) ascending).
OCVAR_HD int group_rank(const int* off, const int* members, int g, int t) {
    int lo = off[g], hi = off[g + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (members[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo - off[g];
}

// The shift of candidate t of a square with matches m[0..n): every matched template t' <= t rotates the corners once more.
OCVAR_HD int prefix_shift(const int* m, int n, const int* off, const int* members, int t) {
    int s = 0;
    for (int k = 0; k < n; k++) s += orient_shift(match_orient_of(m[k])) * group_rank(off, members, match_group(m[k]), t);
    return s & 3;
}

// Host-side table of a library (ocvar_hip_set_templates uploads its arrays).
struct Library {
    std::vector<SizeClass> sizes;
    std::vector<LutEntry> lut;
    std::vector<int> group_off;   // [n_groups + 1] into members
    std::vector<int> members;     // [n] templates of each group, ascending
    std::vector<int> group_of;    // [n] template -> group
    std::vector<int> size_of;     // [n] template -> size class
    std::vector<int> group_size;  // [n_groups] group -> size class
    int max_match = 0;            // most matches one square can have: sum over size classes of the longest run of one code
    int n_groups() const { return (int)group_size.size(); }
};

// false: more than MAX_SIZE_CLASSES distinct sizes.
inline bool build_library(const TemplateRec* t, int n, Library* L) {
    *L = Library();
    L->group_of.assign(n, -1);
    L->size_of.assign(n, -1);
    std::map<std::pair<int, int>, int> size_index;
    std::map<std::vector<long long>, int> group_index;   // key: width, height, code[0..3]
    std::vector<std::vector<int>> groups;
    for (int i = 0; i < n; i++) {
        const auto sk = std::make_pair(t[i].width, t[i].height);
        auto s = size_index.find(sk);
        if (s == size_index.end()) {
            if ((int)L->sizes.size() == MAX_SIZE_CLASSES) return false;
            s = size_index.emplace(sk, (int)L->sizes.size()).first;
            L->sizes.push_back(SizeClass{t[i].width, t[i].height, 0, 0});
        }
        L->size_of[i] = s->second;
        const std::vector<long long> gk = {t[i].width, t[i].height, t[i].code[0], t[i].code[1], t[i].code[2], t[i].code[3]};
        auto g = group_index.find(gk);
        if (g == group_index.end()) {
            g = group_index.emplace(gk, (int)groups.size()).first;
            groups.emplace_back();
            L->group_size.push_back(s->second);
        }
        groups[g->second].push_back(i);
        L->group_of[i] = g->second;
    }
    L->group_off.push_back(0);
    for (const auto& g : groups) {
        L->members.insert(L->members.end(), g.begin(), g.end());
        L->group_off.push_back((int)L->members.size());
    }
    std::vector<std::vector<LutEntry>> per_size(L->sizes.size());
    for (int g = 0; g < (int)groups.size(); g++) {
        const TemplateRec& r = t[groups[g][0]];
        for (int k = 0; k < 4; k++) {
            bool dup = false;   // a symmetric code matches at its first k (match_orient)
            for (int j = 0; j < k; j++) dup = dup || r.code[j] == r.code[k];
            if (!dup) per_size[L->group_size[g]].push_back(LutEntry{r.code[k], g, k + 1});
        }
    }
    for (size_t s = 0; s < per_size.size(); s++) {
        auto& e = per_size[s];
        std::sort(e.begin(), e.end(), [](const LutEntry& a, const LutEntry& b) { return a.code != b.code ? a.code < b.code : a.group < b.group; });
        L->sizes[s].lut_begin = (int)L->lut.size();
        L->sizes[s].lut_count = (int)e.size();
        int longest = 0;
        for (size_t a = 0, b; a < e.size(); a = b) {
            for (b = a; b < e.size() && e[b].code == e[a].code; b++) {}
            longest = std::max(longest, (int)(b - a));
        }
        L->max_match += longest;
        L->lut.insert(L->lut.end(), e.begin(), e.end());
    }
    return true;
}

}  // namespace ocvar
