// dense_emul.cpp -- host build of the dense tail's cores (opencv-ar_amd/csrc/tail_core.h) for tests/test_dense_cpu.py: the
// literal tracking loop against its sparse replay, and the rank rule of cvarFindSquares' order against the chunked sort.
#include "tail_core.h"
#include <algorithm>
#include <cstring>
#include <vector>

using namespace ocvar;

extern "C" {

// track_markers as order_and_crops_kernel runs it: squares compacted in place, markers' squares updated
int dense_track_literal(MarkerRec* markers, int n_markers, float* squares, int n_quads, int* reserve, int max_reserve, int* n_reserve) {
    return track_markers(markers, n_markers, squares, n_quads, reserve, max_reserve, n_reserve);
}

// the sparse replay as track_replay_kernel runs it: grid over a w x h px frame, replay, then the list compacted into out
int dense_track_sparse(MarkerRec* markers, int n_markers, const float* squares, int n_quads, int w, int h, float* out, int* reserve,
                       int max_reserve, int* n_reserve) {
    int gw, gh;
    const int nc = track_grid_cells(w, h, &gw, &gh);
    std::vector<int> cells(nc + 1), items(4 * (size_t)n_quads + 1), next(n_quads + 1);
    track_grid_build(squares, n_quads, gw, gh, cells.data(), items.data());
    const int left = track_markers_sparse(markers, n_markers, squares, n_quads, cells.data(), items.data(), gw, gh, next.data(),
                                          reserve, max_reserve, n_reserve);
    int o = 0;
    for (int i = 0; i < n_quads; i++)
        if (next[i] == i) {
            for (int k = 0; k < 8; k++) out[8 * o + k] = squares[8 * i + k];
            o++;
        }
    return o == left ? left : -1;
}

// Every list of up to max_m markers drawn from pool_m (np_m squares) and up to max_n squares drawn from pool_s (np_s squares),
// with repetition, through both loops on a w x h frame.  Returns the number of lists whose results differ (reserve, count,
// compacted squares, updated marker squares: bitwise); *cases: how many lists were run.
long long dense_track_exhaustive(const float* pool_m, int np_m, int max_m, const float* pool_s, int np_s, int max_n, int w, int h,
                                 long long* cases) {
    long long bad = 0, n_cases = 0;
    std::vector<int> im(max_m), is(max_n);
    for (int nm = 0; nm <= max_m; nm++) {
        long long combos_m = 1;
        for (int k = 0; k < nm; k++) combos_m *= np_m;
        for (long long cm = 0; cm < combos_m; cm++) {
            long long t = cm;
            for (int k = 0; k < nm; k++, t /= np_m) im[k] = (int)(t % np_m);
            for (int n = 0; n <= max_n; n++) {
                long long combos_s = 1;
                for (int k = 0; k < n; k++) combos_s *= np_s;
                for (long long cs = 0; cs < combos_s; cs++) {
                    long long u = cs;
                    for (int k = 0; k < n; k++, u /= np_s) is[k] = (int)(u % np_s);
                    MarkerRec a[8], b[8];
                    std::vector<float> sa(8 * (size_t)n + 8), sb(8 * (size_t)n + 8), out(8 * (size_t)n + 8);
                    for (int k = 0; k < nm; k++) {
                        std::memset(&a[k], 0, sizeof a[k]);
                        for (int q = 0; q < 8; q++) a[k].square[q] = pool_m[8 * im[k] + q];
                        b[k] = a[k];
                    }
                    for (int k = 0; k < n; k++)
                        for (int q = 0; q < 8; q++) sa[8 * k + q] = sb[8 * k + q] = pool_s[8 * is[k] + q];
                    int ra[64], rb[64], nra = 0, nrb = 0;
                    const int la = track_markers(a, nm, sa.data(), n, ra, 64, &nra);
                    const int lb = dense_track_sparse(b, nm, sb.data(), n, w, h, out.data(), rb, 64, &nrb);
                    bool same = la == lb && nra == nrb && std::memcmp(ra, rb, sizeof(int) * (nra < 64 ? nra : 64)) == 0 &&
                                std::memcmp(sa.data(), out.data(), sizeof(float) * 8 * (la > 0 ? la : 0)) == 0;
                    for (int k = 0; k < nm; k++) same = same && std::memcmp(a[k].square, b[k].square, sizeof a[k].square) == 0;
                    bad += !same;
                    n_cases++;
                }
            }
        }
    }
    *cases = n_cases;
    return bad;
}

// slot of square i under the rank rule of order_and_crops_kernel
void dense_order_rank(const int* start, int n, int* slot) {
    for (int i = 0; i < n; i++) {
        int r = 0;
        for (int u = 0; u < n; u++) r += start[u] > start[i];
        slot[i] = r;
    }
}

// the same through order_sort_kernel (bitonic network per chunk of `chunk` starts, padded with INT_MAX) and order_place_kernel
void dense_order_sorted(const int* start, int n, int chunk, int* slot) {
    std::vector<int> sorted(n > 0 ? n : 1), key(chunk);
    for (int lo = 0; lo < n; lo += chunk) {
        const int len = std::min(chunk, n - lo);
        for (int k = 0; k < chunk; k++) key[k] = k < len ? start[lo + k] : 0x7fffffff;
        for (int k = 2; k <= chunk; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1)
                for (int tid = 0; tid < chunk / 2; tid++) bitonic_step(key.data(), k, j, tid);
        for (int k = 0; k < len; k++) sorted[lo + k] = key[k];
    }
    for (int i = 0; i < n; i++) {
        int r = 0;
        for (int b = 0; b < n; b += chunk) r += count_greater_sorted(sorted.data() + b, std::min(chunk, n - b), start[i]);
        slot[i] = r;
    }
}

int dense_order_chunk() { return ORDER_CHUNK; }

}  // extern "C"
