// decode.hip -- per-quad code readout and the per-frame tail (dedupe, pose, marker records) on gfx950.
//
// decode_kernel replaces the inner template loop of cvarArMultRegistration
// (/root/reference/src/opencvar.cpp:700-774) for one frame-pass quad per wave.  The reference re-runs the whole
// square finder on the crop once per template with an identical result; here the crop pass ran
// once and every template reads the same crop quad.  The read code depends on a template only through its size, so a
// square is read once per size class and the code is looked up in the library's sorted table (library_core.h): the work per
// square grows with the number of sizes and of matches, not with the number of templates.  What decode keeps per square is
// compact (SquareRec, one code per size class, the matched groups); the reference's K candidates per square are implied by it
// (ocvar_hip_debug_candidates spells them out on the host).
// finalise_kernel replaces opencvar.cpp:662-668 and 780-801 for one frame per workgroup (the order-dependent elimination in
// its sparse form, tail_core.h, and the marker records); pose_kernel solves the survivors' poses (cvarSquareToMatrix
// 524-540), one lane per marker over the whole batch.
#include "kernels.h"

namespace ocvar {

// One wave per (frame, quarter of the frame's quads): workgroups of 64 threads, because with several contexts in flight a
// workgroup has to fit into the gap one retiring binarise wave leaves (round 2's 256-thread workgroups at 128 registers took 5 ms
// in-region for 0.3 ms of work).  Four phases per chunk of 8 quads.  Phase 1, one lane per (quad, size class): the inverse
// homography (closed form in double, rounded to float32 and inverted; the destination quad is (tw+2) x (th+2), so it depends on
// the size) into LDS.  Phase 2, quad by quad, one lane per code cell: lane L samples the cell whose bit is bit L of the
// code -- acArray2DToBit packs row-major, columns right to left, first cell in the most significant bit (acmath.cpp:546-554)
// -- so the code is the ballot of the thresholded samples.  Phase 3, one lane per (quad, size class): the code's run in the
// size class's table.  Phase 4, one lane per quad: the runs merged into the quad's match list, ascending by group (= by
// first template).
constexpr int DECODE_SLICES = 4;   // waves per frame: quad i belongs to slice i % 4
constexpr int DECODE_CHUNK = 8;    // quads of a slice per round (x size classes <= 128 lanes of phases 1 and 3)

template <bool DENSE>
__global__ __launch_bounds__(64) void decode_kernel(Workspace ws) {
    extern __shared__ double sM_dyn[];   // [DECODE_CHUNK][n_sizes][9]
    __shared__ int s_roi[DECODE_CHUNK];        // crop ROI of the chunk's quad, -1: no quad in its crop
    __shared__ unsigned s_slot[DECODE_CHUNK];  // quads_crop slot of the crop's quad
    __shared__ long long s_code[DECODE_CHUNK * MAX_SIZE_CLASSES];
    __shared__ int s_lo[DECODE_CHUNK * MAX_SIZE_CLASSES], s_cnt[DECODE_CHUNK * MAX_SIZE_CLASSES];
    // (dense contexts: more waves per frame, ws.decode_slices -- thousands of squares would queue behind four)
    const int SLICES = DENSE ? ws.decode_slices : DECODE_SLICES;
    const int f = blockIdx.x / SLICES, slice = blockIdx.x % SLICES;
    const int lane = threadIdx.x;
    const int NS = ws.n_sizes;
    int nsq = ws.n_squares[f];
    nsq = nsq < ws.maxq ? nsq : ws.maxq;
    const int mine = (nsq - slice + SLICES - 1) / SLICES;   // quads slice, slice + SLICES, ... < nsq
    for (int base = 0; base < mine; base += DECODE_CHUNK) {
        const int cnt = mine - base < DECODE_CHUNK ? mine - base : DECODE_CHUNK;
        if (lane < cnt) {
            const int i = slice + SLICES * (base + lane);
            const int r = ws.crop_of[(size_t)f * ws.maxq + i];
            unsigned long long best = ~0ull;
            if (r >= 0) best = ws.best_crop[r];
            s_roi[lane] = best == ~0ull ? -1 : r;
            s_slot[lane] = (unsigned)(best & 0xffffffffu);
        }
        __syncthreads();
        for (int pair = lane; pair < cnt * NS; pair += 64) {
            const int qi = pair / NS, s = pair - qi * NS;
            if (s_roi[qi] < 0) continue;
            const QuadRec q = ws.quads_crop[s_slot[qi]];
            float pat[8], m32[9];
            for (int k = 0; k < 8; k++) pat[k] = (float)q.pt[k];
            const SizeClass sz = ws.sizes[s];
            if (!perspective_from_quad(pat, sz.width + 2, sz.height + 2, m32))
                for (int k = 0; k < 9; k++) m32[k] = 0.f;
            double M[9];
            invert_map(m32, M);
            for (int k = 0; k < 9; k++) sM_dyn[(qi * NS + s) * 9 + k] = M[k];
        }
        __syncthreads();
        for (int qi = 0; qi < cnt; qi++) {
            const int i = slice + SLICES * (base + qi);
            SquareRec* rec = ws.sq_recs + (size_t)f * ws.maxq + i;
            const int r = s_roi[qi];
            if (r < 0) {  // no quad in the crop: no candidate for this square (opencvar.cpp:704)
                if (lane == 0) rec->n_match = -1;
                continue;
            }
            const Roi roi = ws.rois_crop[r];
            if (lane < 8) rec->square[lane] = ws.squares[((size_t)f * ws.maxq + i) * 8 + lane];
            else if (lane < 16) rec->patPoint[lane - 8] = (float)ws.quads_crop[s_slot[qi]].pt[lane - 8];
            const uint8_t* plane = ws.gray + (size_t)roi.frame * gray_plane_bytes(ws.W, ws.H);
            const int pitch = gray_pitch(ws.W);
            auto crop_px = [=](int ix, int iy) -> int { return plane[(size_t)(roi.y0 + iy) * pitch + gray_col(roi.x0 + ix)]; };
            for (int s = 0; s < NS; s++) {
                const SizeClass sz = ws.sizes[s];
                double M[9];
                for (int k = 0; k < 9; k++) M[k] = sM_dyn[(qi * NS + s) * 9 + k];
                const int n = sz.width * sz.height;     // <= 64 (ocvar_hip_set_templates)
                bool v = false;
                if (lane < n) {
                    const int p = n - 1 - lane;       // position in acArray2DToBit's scan: row p / tw, column tw-1 - p % tw
                    const int ci = p / sz.width, cj = sz.width - 1 - p % sz.width;
                    int cx, cy;
                    if (code_cell(ci * sz.width + cj, sz.width, sz.height, &cx, &cy))
                        v = warp_sample_px(crop_px, roi.w, roi.h, M, cx + 1, cy + 1) > 100;
                }
                const long long bit = (long long)__ballot(v);
                if (lane == 0) s_code[qi * MAX_SIZE_CLASSES + s] = bit;
            }
        }
        __syncthreads();
        for (int pair = lane; pair < cnt * NS; pair += 64) {
            const int qi = pair / NS, s = pair - qi * NS;
            if (s_roi[qi] < 0) continue;
            const int i = slice + SLICES * (base + qi);
            const long long bit = s_code[qi * MAX_SIZE_CLASSES + s];
            ws.sq_codes[((size_t)f * ws.maxq + i) * NS + s] = bit;
            const SizeClass sz = ws.sizes[s];
            int n;
            s_lo[qi * MAX_SIZE_CLASSES + s] = lut_find(ws.lut, sz.lut_begin, sz.lut_count, bit, &n);
            s_cnt[qi * MAX_SIZE_CLASSES + s] = n;
        }
        __syncthreads();
        if (lane < cnt && s_roi[lane] >= 0) {
            const int i = slice + SLICES * (base + lane);
            int* out = ws.sq_match + ((size_t)f * ws.maxq + i) * ws.max_match;
            int n = 0;   // <= max_match: at most the longest run of one code per size class
            for (int s = 0; s < NS; s++) {
                const int lo = s_lo[lane * MAX_SIZE_CLASSES + s], hi = lo + s_cnt[lane * MAX_SIZE_CLASSES + s];
                for (int e = lo; e < hi; e++) {   // (runs of different size classes interleave in group order)
                    const LutEntry le = ws.lut[e];
                    n = insert_match(out, n, le.group << 2 | (le.orient - 1));
                }
            }
            ws.sq_recs[(size_t)f * ws.maxq + i].n_match = n;
        }
        __syncthreads();
    }
}

// The elimination in its sparse form (tail_core.h: square_survivor), one wave per frame.  Pass 1: the first square matching
// each group (LDS atomicMin over the frame's matches); pass 2, one lane per square: its survivor; then the survivors in
// square order behind the tracked markers.  LDS: n_groups + maxq ints, sized at launch.
// Dense contexts (DENSE): s_surv and s_src live in global workspace (ws.surv, ws.src), the LDS holds n_groups ints only.
template <bool DENSE>
__global__ __launch_bounds__(64) void finalise_kernel(Workspace ws) {
    extern __shared__ int tail_lds[];
    __shared__ int s_src_lds[DENSE ? 1 : MAXM];
    const int f = blockIdx.x;
    const int MM_OUT = DENSE ? ws.maxm : MAXM;   // marker records per frame
    int* s_earliest = tail_lds;                // [n_groups]
    // [maxq] template << 1 | score of the square's survivor, -1: none
    int* s_surv = DENSE ? ws.surv + (size_t)f * ws.maxq : tail_lds + ws.n_groups;
    int* s_src = DENSE ? ws.src + (size_t)f * ws.maxm : s_src_lds;   // >= 0: square index, < 0: -(1 + index into prev)
    __shared__ int s_first, s_nout, s_job;
    const int lane = threadIdx.x;   // one wave per frame
    int nsq = ws.n_squares[f];
    nsq = nsq < ws.maxq ? nsq : ws.maxq;
    const SquareRec* recs = ws.sq_recs + (size_t)f * ws.maxq;
    const int MM = ws.max_match;
    const int* match = ws.sq_match + (size_t)f * ws.maxq * MM;
    for (int g = lane; g < ws.n_groups; g += 64) s_earliest[g] = NO_SQUARE;
    if (lane == 0) s_first = NO_SQUARE;
    __syncthreads();
    for (int i = lane; i < nsq; i += 64) {
        const int n = recs[i].n_match;
        if (n >= 0) atomicMin(&s_first, i);
        for (int k = 0; k < n; k++) atomicMin(&s_earliest[match_group(match[(size_t)i * MM + k])], i);
    }
    __syncthreads();
    for (int i = lane; i < nsq; i += 64) {
        const int n = recs[i].n_match;
        int v = -1;
        if (n >= 0) {
            int score;
            const int t = square_survivor(i, i == s_first, n, match + (size_t)i * MM, s_earliest, ws.group_off, ws.group_members, &score);
            if (t >= 0) v = t << 1 | score;
        }
        s_surv[i] = v;
    }
    __syncthreads();
    if (DENSE) {
        // the same list, compacted by the whole wave (ballot + prefix count) instead of one lane walking thousands of squares
        const int nr = ws.n_reserve[f];
        for (int k = lane; k < nr && k < MM_OUT; k += 64) s_src[k] = -(1 + ws.reserve[(size_t)f * MM_OUT + k]);
        int total = nr;
        for (int base = 0; base < nsq; base += 64) {
            const int i = base + lane;
            const bool v = i < nsq && s_surv[i] >= 0;
            const unsigned long long b = __ballot(v);
            const int pos = total + __popcll(b & ((1ull << lane) - 1ull));
            if (v && pos < MM_OUT) s_src[pos] = i;
            total += __popcll(b);
        }
        if (lane == 0) {
            const int nout = total < MM_OUT ? total : MM_OUT;
            s_nout = nout;
            if (total > MM_OUT) atomicOr(ws.counters + CNT_ERR, ERR_MARKER_OVERFLOW);
            ws.n_markers[f] = total;
            s_job = nout > 0 ? atomicAdd(ws.counters + CNT_POSE_JOBS, nout) : 0;
        }
    } else if (lane == 0) {
        int nout = 0, total = 0;
        const int nr = ws.n_reserve[f];
        for (int k = 0; k < nr; k++) {  // tracked markers first (662-668)
            if (k < MM_OUT && nout < MM_OUT) s_src[nout++] = -(1 + ws.reserve[(size_t)f * MM_OUT + k]);
            total++;
        }
        for (int i = 0; i < nsq; i++)
            if (s_surv[i] >= 0) {
                if (nout < MM_OUT) s_src[nout++] = i;
                total++;
            }
        s_nout = nout;
        // more markers than a frame's output block holds (tracking keeps duplicates, opencvar.cpp:662-668): the next frame's
        // `prev` would be cut short and its tracking would diverge from the reference -- fail loudly instead
        if (total > MM_OUT) atomicOr(ws.counters + CNT_ERR, ERR_MARKER_OVERFLOW);
        ws.n_markers[f] = total;
        s_job = nout > 0 ? atomicAdd(ws.counters + CNT_POSE_JOBS, nout) : 0;   // one list append per frame
    }
    __syncthreads();
    // the surviving markers' records, all but the pose; one pose job per marker for pose_kernel
    for (int k = threadIdx.x; k < s_nout; k += blockDim.x) {
        MarkerRec* m = ws.markers + (size_t)f * MM_OUT + k;
        const int src = s_src[k];
        if (src < 0) {
            *m = ws.prev[(size_t)f * MM_OUT + (-src - 1)];  // square already updated by the tracking step
        } else {
            const int i = src, t = s_surv[i] >> 1;
            const int sh = prefix_shift(match + (size_t)i * MM, recs[i].n_match, ws.group_off, ws.group_members, t);
            float sq[8];
            for (int q = 0; q < 8; q++) sq[q] = recs[i].square[q];
            const TemplateRec tp = ws.templates[t];
            m->templateId = t;
            m->markerId = i;
            m->score = (s_surv[i] & 1) ? 1.0 : 0.0;
            shift_square(sq, sh, m->square);
            m->aspectRatio = (double)tp.width / tp.height;
        }
        ws.pose_jobs[s_job + k] = f * MM_OUT + k;
    }
}

// cvarSquareToMatrix (opencvar.cpp:524-540) for every surviving marker of the batch, one lane each.  Round 2 solved the poses
// inside the per-frame tail kernel: one 64-lane workgroup per frame with at most 3 lanes in the solver, capped at 128 registers so
// that it could start between binarise waves -- the solver's arrays lived in scratch memory and the kernel took 1.06 ms per
// 2048 frames for ~5 k poses.  Here the ~5 k jobs fill ~85 waves, every array of the solver is a register (loops unrolled to
// constant indices, the seeding homography in closed form: pose_core.h) and the kernel is as long as one solve.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void pose_kernel(Workspace ws) {
    int n = ws.counters[CNT_POSE_JOBS];
    const int cap = ws.n_frames * ws.maxm;
    if (n > cap) n = cap;
    const CameraRec cam = *ws.camera;
    for (int j = blockIdx.x * 64 + threadIdx.x; j < n; j += gridDim.x * 64) {
        MarkerRec* m = ws.markers + ws.pose_jobs[j];
        float sq[8];
        for (int q = 0; q < 8; q++) sq[q] = m->square[q];
        double gl[16];
        square_to_glmatrix(sq, cam, m->aspectRatio, gl);
        for (int q = 0; q < 16; q++) m->glMatrix[q] = gl[q];
    }
}

void launch_decode(const Workspace& ws, hipStream_t stream) {
    if (ws.n_frames <= 0) return;
    const size_t lds = (size_t)DECODE_CHUNK * ws.n_sizes * 9 * sizeof(double);
    if (ws.dense) hipLaunchKernelGGL(decode_kernel<true>, dim3(ws.n_frames * ws.decode_slices), dim3(64), lds, stream, ws);
    else hipLaunchKernelGGL(decode_kernel<false>, dim3(ws.n_frames * DECODE_SLICES), dim3(64), lds, stream, ws);
}
void launch_finalise(const Workspace& ws, const RefineArgs& refine, hipStream_t stream) {
    if (ws.n_frames <= 0) return;
    // a stateless frame keeps at most one marker per template: a grid of one wave per 8 frames takes a batch's poses in one
    // pass; stateful batches with many tracked markers per frame loop (grid-stride).  A dense context sizes the grid for its
    // marker records (one lane each, up to 2048 waves)
    int blocks = ws.n_frames / 8 + 1;
    if (ws.dense) {
        hipLaunchKernelGGL(finalise_kernel<true>, dim3(ws.n_frames), dim3(64), (size_t)ws.n_groups * sizeof(int), stream, ws);
        const long long want = ((long long)ws.n_frames * ws.maxm + 63) / 64;
        blocks = (int)(want < 2048 ? (want > blocks ? want : blocks) : 2048);
    } else {
        hipLaunchKernelGGL(finalise_kernel<false>, dim3(ws.n_frames), dim3(64), (size_t)(ws.n_groups + ws.maxq) * sizeof(int), stream, ws);
    }
    if (refine.half_win > 0) launch_refine_corners(ws, refine, stream);
    hipLaunchKernelGGL(pose_kernel, dim3(blocks), dim3(64), 0, stream, ws);
}

}  // namespace ocvar
