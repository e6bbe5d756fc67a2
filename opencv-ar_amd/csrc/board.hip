// board.hip -- opt-in pose of one planar marker board per frame (ocvar_hip_set_board), after launch_finalise (marker records,
// refined corners and poses) and before the copy-out.  The rules, the summation order and the reduction tree are board_core.h's;
// its host build (tests/emul/board_emul.cpp) reproduces this kernel's selection and counts bit for bit.
#include "kernels.h"
#include <limits.h>

namespace ocvar {

// The device's sums: this lane's partial (board_partial), then a butterfly of shuffles over the wave, which leaves board_tree's
// value in all 64 lanes.
template <bool DIST>
struct BoardSumsDev {
    const BoardObs* obs;
    int n;
    const BoardEntry* entries;
    double fx, fy, cx, cy;
    const double* dist;
    int lane;
    OCVAR_D void jac(const double* p, double* S) const {
        board_partial<true, DIST>(obs, n, entries, p, fx, fy, cx, cy, dist, lane, S);
        for (int mask = BOARD_LANES / 2; mask >= 1; mask >>= 1)
            OCVAR_UNROLL
            for (int q = 0; q < BOARD_SUMS; q++) S[q] = S[q] + __shfl_xor(S[q], mask, BOARD_LANES);
    }
    OCVAR_D double err(const double* p) const {
        double s[1];
        board_partial<false, DIST>(obs, n, entries, p, fx, fy, cx, cy, dist, lane, s);
        for (int mask = BOARD_LANES / 2; mask >= 1; mask >>= 1) s[0] = s[0] + __shfl_xor(s[0], mask, BOARD_LANES);
        return s[0];
    }
};

// One wave per frame.  Phase 1: the lanes scan the frame's records (an LDS atomicMin per board entry keeps the first record
// index), one lane per chosen record reads its code again (board_read_rotation), and the used observations are compacted into
// LDS in board-index order (ballot + popcount).  Phase 2: every lane runs the same seeds and Levenberg-Marquardt steps; each
// lane's share of the corners is summed over the wave by the butterfly.  Board coordinates come from the global table.
__global__ __launch_bounds__(64) void board_pose_kernel(Workspace ws, BoardArgs ba) {
    __shared__ int s_first[BOARD_MAX];
    __shared__ BoardObs s_obs[BOARD_MAX];
    __shared__ double s_area[BOARD_MAX];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int nb = ba.n;
    for (int b = lane; b < nb; b += BOARD_LANES) s_first[b] = INT_MAX;
    __syncthreads();
    int nrec = ws.n_markers[f];
    if (nrec > ws.maxm) nrec = ws.maxm;
    const MarkerRec* recs = ws.markers + (size_t)f * ws.maxm;
    for (int k = lane; k < nrec; k += BOARD_LANES) {
        const int b = board_slot(recs[k], ba.map, ws.templates, ws.n_templates);
        if (b >= 0 && b < nb) atomicMin(&s_first[b], k);
    }
    __syncthreads();
    const int W = ws.W, H = ws.H, pitch = gray_pitch(ws.W);
    const uint8_t* plane = ws.gray + (size_t)f * gray_plane_bytes(ws.W, ws.H);
    auto px = [=](int x, int y) -> int { return plane[(size_t)y * pitch + gray_col(x)]; };
    int n = 0;
    for (int b0 = 0; b0 < nb; b0 += BOARD_LANES) {
        const int b = b0 + lane;
        BoardObs o;
        bool ok = false;
        if (b < nb && s_first[b] != INT_MAX) {
            const MarkerRec& m = recs[s_first[b]];
            const int k = board_read_rotation(px, W, H, m.square, ws.templates[m.templateId]);
            if (k >= 0) {
                board_observe(m, b, k, o);
                ok = true;
            }
        }
        const unsigned long long used = __ballot(ok);
        if (ok) {
            const int pos = n + __popcll(used & ((1ull << lane) - 1ull));
            s_obs[pos] = o;
            s_area[pos] = board_quad_area(o.sq);
        }
        n += __popcll(used);
    }
    __syncthreads();
    const CameraRec cam = *ws.camera;
    double fx, fy, cx, cy, kd[5];
    const bool dist = board_camera(cam, &fx, &fy, &cx, &cy, kd);
    BoardPose out;
    if (dist) board_solve_t<true>(BoardSumsDev<true>{s_obs, n, ba.entries, fx, fy, cx, cy, kd, lane}, s_obs, s_area, n, ba.entries, fx, fy, cx, cy, kd, out);
    else board_solve_t<false>(BoardSumsDev<false>{s_obs, n, ba.entries, fx, fy, cx, cy, kd, lane}, s_obs, s_area, n, ba.entries, fx, fy, cx, cy, kd, out);
    if (lane == 0) ba.poses[f] = out;
}

void launch_board_poses(const Workspace& ws, const BoardArgs& board, hipStream_t stream) {
    if (ws.n_frames <= 0 || board.n <= 0) return;
    hipLaunchKernelGGL(board_pose_kernel, dim3(ws.n_frames), dim3(BOARD_LANES), 0, stream, ws, board);
}

}  // namespace ocvar
