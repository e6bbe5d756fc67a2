// flow.hip -- opt-in flow tracking of marker records between two blocks of device-resident frames (ocvar_hip_flow_records).
// The definition is flow_core.h's; its host build (tests/emul/flow_emul.cpp) gives these kernels' bytes.  Three kernels on one
// stream: flow_grey_kernel (level 0 of every frame of a chunk), flow_down_kernel once per level (a level is complete when the next
// launch reads it: stream order, no flags between workgroups), flow_track_kernel.  Parameters, pyramid layout and camera travel by
// value in the launch arguments.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int FLOW_LANE_PX = 4;                   // consecutive pixels of one row a lane owns: one dword of a level
constexpr int FLOW_WAVE_PX = 64 * FLOW_LANE_PX;   // a wave's span: 256 bytes at a 256-byte boundary of the level's row -- whole sectors,
                                                  // rows being a multiple of 64 bytes apart (flow_geom)

// Level 0.  A one-wave workgroup owns a span of one row (blockIdx: span, row, frame).  ALIGNED (the frames' address, row stride and
// frame stride are multiples of 4): a lane's 4 BPP source bytes are BPP whole dwords and loaded as such, except in the lane that
// crosses the row's end; everything else is read byte by byte.  The bytes behind the row's end inside the lane's dword are 0.
template <int BPP, bool ALIGNED>
__global__ __launch_bounds__(64) void flow_grey_kernel(FlowPyrArgs a, int fmt) {
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * FLOW_LANE_PX;
    const int y = blockIdx.y, W = a.g.w[0];
    if (x0 >= W) return;
    const uint8_t* src = a.frames + (size_t)blockIdx.z * a.frame_stride + (long long)y * a.row_stride + (long long)x0 * BPP;
    unsigned out = 0;
    if (ALIGNED && x0 + FLOW_LANE_PX <= W) {
        const unsigned* s4 = reinterpret_cast<const unsigned*>(src);
        unsigned q[BPP];
        OCVAR_UNROLL
        for (int j = 0; j < BPP; j++) q[j] = s4[j];
        OCVAR_UNROLL
        for (int i = 0; i < FLOW_LANE_PX; i++) {
            uint8_t px[BPP];
            OCVAR_UNROLL
            for (int c = 0; c < BPP; c++) px[c] = (uint8_t)run_byte(q, i * BPP + c);
            out |= (unsigned)flow_grey(px, fmt) << (8 * i);
        }
    } else {
        OCVAR_UNROLL
        for (int i = 0; i < FLOW_LANE_PX; i++)
            if (x0 + i < W) out |= (unsigned)flow_grey(src + i * BPP, fmt) << (8 * i);
    }
    uint8_t* dst = a.pyr + (size_t)blockIdx.z * a.slot_bytes + a.g.off[0] + (long long)y * a.g.pitch[0] + x0;
    *reinterpret_cast<unsigned*>(dst) = out;   // (x0 + 3 < pitch: the pitch is a multiple of 64 above x0)
}

// Level l + 1 from level l: the same spans over the destination's rows.  A lane's four pixels need the source columns 2 x0 - 2 ..
// 2 x0 + 8 of five rows; inside the row they are bytes 2 .. 12 of four aligned dwords, at the row's ends they are read one by one
// through the reflection.  Integer sums: the order does not matter.
__global__ __launch_bounds__(64) void flow_down_kernel(uint8_t* pyr, long long slot_bytes, FlowGeom g, int l) {
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * FLOW_LANE_PX;
    const int y = blockIdx.y, Ws = g.w[l], Hs = g.h[l], Wd = g.w[l + 1];
    if (x0 >= Wd) return;
    uint8_t* base = pyr + (size_t)blockIdx.z * slot_bytes;
    const uint8_t* src = base + g.off[l];
    const int sp = g.pitch[l];
    const bool inside = 2 * x0 - 4 >= 0 && 2 * x0 + 8 < Ws;   // (then 2 x0 + 11 < sp, and all four pixels exist)
    int acc[FLOW_LANE_PX] = {0, 0, 0, 0};
    OCVAR_UNROLL
    for (int j = 0; j < 5; j++) {
        const uint8_t* r = src + (long long)flow_reflect(2 * y + j - 2, Hs) * sp;
        int c[11];
        if (inside) {
            const unsigned* r4 = reinterpret_cast<const unsigned*>(r + 2 * x0 - 4);
            const unsigned q[4] = {r4[0], r4[1], r4[2], r4[3]};
            OCVAR_UNROLL
            for (int t = 0; t < 11; t++) c[t] = run_byte(q, t + 2);
        } else {
            OCVAR_UNROLL
            for (int t = 0; t < 11; t++) c[t] = r[flow_reflect(2 * x0 - 2 + t, Ws)];
        }
        OCVAR_UNROLL
        for (int o = 0; o < FLOW_LANE_PX; o++)
            acc[o] += flow_k(j) * (c[2 * o] + 4 * c[2 * o + 1] + 6 * c[2 * o + 2] + 4 * c[2 * o + 3] + c[2 * o + 4]);
    }
    unsigned out = 0;
    OCVAR_UNROLL
    for (int o = 0; o < FLOW_LANE_PX; o++)
        if (x0 + o < Wd) out |= (unsigned)((acc[o] + 128) >> 8) << (8 * o);
    *reinterpret_cast<unsigned*>(base + g.off[l + 1] + (long long)y * g.pitch[l + 1] + x0) = out;
}

template <int BPP>
static void launch_grey(const FlowPyrArgs& a, int n_frames, int format, bool aligned, hipStream_t stream) {
    const dim3 grid((a.g.w[0] + FLOW_WAVE_PX - 1) / FLOW_WAVE_PX, a.g.h[0], n_frames);
    if (aligned)
        hipLaunchKernelGGL((flow_grey_kernel<BPP, true>), grid, dim3(64), 0, stream, a, format);
    else
        hipLaunchKernelGGL((flow_grey_kernel<BPP, false>), grid, dim3(64), 0, stream, a, format);
}

void launch_flow_pyramids(const FlowPyrArgs& a, int n_frames, int format, hipStream_t stream) {
    if (n_frames <= 0 || a.g.w[0] <= 0 || a.g.h[0] <= 0) return;
    const bool aligned = frames_dwords(a.frames, a.row_stride, a.frame_stride);
    switch (format_bpp(format)) {
        case 1: launch_grey<1>(a, n_frames, format, aligned, stream); break;
        case 3: launch_grey<3>(a, n_frames, format, aligned, stream); break;
        case 4: launch_grey<4>(a, n_frames, format, aligned, stream); break;
        default: return;
    }
    for (int l = 0; l < a.g.L; l++) {
        const dim3 grid((a.g.w[l + 1] + FLOW_WAVE_PX - 1) / FLOW_WAVE_PX, a.g.h[l + 1], n_frames);
        hipLaunchKernelGGL(flow_down_kernel, grid, dim3(64), 0, stream, a.pyr, a.slot_bytes, a.g, l);
    }
}

// flow_track_forward for the four corners of one record at once: one 16-lane row per corner (row-uniform: px, py, run and
// everything returned).  A row samples its patches into its part of LDS (I, J), takes its partial sums and combines them with a
// butterfly of shuffles inside the row, which leaves flow_tree's value in all 16 lanes.  The wave walks the levels together and
// loops over the steps until its rows have stopped: at most max_iter steps per level.  run false: the row sits the call out.
__device__ int flow_track_rows(const uint8_t* A, const uint8_t* B, const FlowGeom& g, const FlowArgs& fa, float px, float py, bool run, float* I,
                               float* J, int lane, float& qx, float& qy, float& err) {
    const int w = fa.half_win;
    qx = px;
    qy = py;
    err = -1.0f;
    int code = !run ? 0 : (flow_inside(px, py, g.w[0], g.h[0]) ? 1 : -1);
    bool alive = code == 1;
    float gx = 0.0f, gy = 0.0f, dx = 0.0f, dy = 0.0f;
    for (int l = g.L; l >= 0; l--) {   // (uniform)
        const float sc = 1.0f / (float)(1 << l);
        const float bx = px * sc + gx, by = py * sc + gy;
        if (alive) refine_sample(flow_level_px(A, g, l), g.w[l], g.h[l], w, px * sc, py * sc, I, lane, FLOW_LANES);
        __syncthreads();
        double s[3] = {0.0, 0.0, 0.0};
        if (alive) flow_grad_partial(I, w, lane, s);
        for (int mask = FLOW_LANES / 2; mask >= 1; mask >>= 1)
            for (int q = 0; q < 3; q++) s[q] = s[q] + __shfl_xor(s[q], mask, FLOW_LANES);
        dx = dy = 0.0f;
        bool active = false;
        if (alive) {
            if (flow_texture(s, w, fa.min_eig)) {
                active = true;
            } else if (l == 0) {
                code = -2;
                alive = false;
            }
        }
        int iter = 0;
        while (__ballot(active) != 0ull) {
            if (active) refine_sample(flow_level_px(B, g, l), g.w[l], g.h[l], w, bx + dx, by + dy, J, lane, FLOW_LANES);
            __syncthreads();
            double e[2] = {0.0, 0.0};
            if (active) flow_diff_partial(I, J, w, lane, e);
            for (int mask = FLOW_LANES / 2; mask >= 1; mask >>= 1)
                for (int q = 0; q < 2; q++) e[q] = e[q] + __shfl_xor(e[q], mask, FLOW_LANES);
            if (active) {
                const bool stop = flow_step(s, e, bx, by, g.w[l], g.h[l], l, fa.eps2, dx, dy, code);
                iter++;
                if (code != 1) alive = false;
                if (stop || iter >= fa.max_iter) active = false;
            }
            __syncthreads();   // (the next step overwrites J)
        }
        if (l > 0) {
            gx = 2.0f * (gx + dx);
            gy = 2.0f * (gy + dy);
        }
        __syncthreads();   // (the next level overwrites I)
    }
    if (alive) {
        qx = (px + gx) + dx;
        qy = (py + gy) + dy;
        refine_sample(flow_level_px(B, g, 0), g.w[0], g.h[0], w, qx, qy, J, lane, FLOW_LANES);
    }
    __syncthreads();
    double a[1] = {0.0};
    if (alive) flow_abs_partial(I, J, w, lane, a);
    for (int mask = FLOW_LANES / 2; mask >= 1; mask >>= 1) a[0] = a[0] + __shfl_xor(a[0], mask, FLOW_LANES);
    if (alive) {
        err = flow_err(a[0], w);
        if (fa.max_err > 0.0f && err > fa.max_err) code = -4;
    }
    __syncthreads();
    return code;
}

constexpr int REC_DWORDS = sizeof(MarkerRec) / 4, REC_SQUARE_DWORD = offsetof(MarkerRec, square) / 4, REC_GL_DWORDS = sizeof(double) * 16 / 4;
static_assert(REC_DWORDS == 46 && REC_SQUARE_DWORD == 36 && offsetof(MarkerRec, glMatrix) == 0, "CvarMarker layout");

// One 64-lane workgroup per record slot (grid-stride over slot and frame), one 16-lane row per corner.  Lanes 0 .. 45 hold the
// record's dwords, read before anything is written (out may be in); nothing that is read or written depends on what the record
// holds: the sampler clamps, a corner outside the frame never starts.
__global__ __launch_bounds__(64) void flow_track_kernel(FlowTrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_flow[];   // [4][2][(2w+3)^2]
    const int side = refine_patch_side(a.fa.half_win), area = side * side;
    const int t = threadIdx.x, row = t >> 4, lane = t & (FLOW_LANES - 1);
    float* I = s_flow + row * 2 * area;
    float* J = I + area;
    const long long total = (long long)a.n_frames * a.slots;
    for (long long j = blockIdx.x; j < total; j += gridDim.x) {   // (uniform across the wave)
        const int f = (int)(j / a.slots), k = (int)(j - (long long)f * a.slots);
        int n = a.counts[f];
        n = n < a.slots ? n : a.slots;
        if (k >= n) {
            if (t == 0 && a.status) a.status[j] = 0;
            continue;
        }
        const MarkerRec* in = a.in + j;
        const unsigned mine = t < REC_DWORDS ? reinterpret_cast<const unsigned*>(in)[t] : 0u;
        const double ratio = in->aspectRatio;
        const float px = in->square[2 * row], py = in->square[2 * row + 1];
        const uint8_t* A = a.pyr_a + (size_t)f * a.slot_bytes;
        const uint8_t* B = a.pyr_b + (size_t)f * a.slot_bytes;
        float qx, qy, err;
        int code = flow_track_rows(A, B, a.g, a.fa, px, py, true, I, J, lane, qx, qy, err);
        if (a.fa.fb_max > 0.0f) {   // (uniform)
            float bx, by, berr;
            const int back = flow_track_rows(B, A, a.g, a.fa, qx, qy, code == 1, I, J, lane, bx, by, berr);
            if (code == 1) code = flow_fb_code(back, bx, by, px, py, a.fa.fb_max);
        }
        int codes[4];
        float sq[8];
        OCVAR_UNROLL
        for (int i = 0; i < 4; i++) {
            codes[i] = __shfl(code, FLOW_LANES * i);
            sq[2 * i] = __shfl(qx, FLOW_LANES * i);
            sq[2 * i + 1] = __shfl(qy, FLOW_LANES * i);
        }
        const int st = flow_record_status(codes, sq);
        // the record's new dword t: the corner (t - 36) / 2 of a tracked record's square, else what was there
        const int corner = (t - REC_SQUARE_DWORD) >> 1;
        const int from = FLOW_LANES * (corner < 0 ? 0 : (corner > 3 ? 3 : corner));
        const float cx = __shfl(qx, from), cy = __shfl(qy, from);
        unsigned v = mine;
        if (st == 1 && t >= REC_SQUARE_DWORD && t < REC_SQUARE_DWORD + 8) v = __float_as_uint((t & 1) ? cy : cx);
        const bool pose = st == 1 && (a.fa.flags & OCVAR_FLOW_POSE) != 0;
        MarkerRec* out = a.out + j;
        if (t < REC_DWORDS && !(pose && t < REC_GL_DWORDS)) reinterpret_cast<unsigned*>(out)[t] = v;
        if (pose && t == 0) {
            double gl[16];
            square_to_glmatrix(sq, a.cam, ratio, gl);
            for (int q = 0; q < 16; q++) out->glMatrix[q] = gl[q];
        }
        if (lane == 0 && a.err) a.err[j * 4 + row] = err;
        if (t == 0 && a.status) a.status[j] = st;
    }
}

void launch_flow_track(const FlowTrackArgs& a, hipStream_t stream) {
    if (a.n_frames <= 0 || a.slots <= 0) return;
    const int side = refine_patch_side(a.fa.half_win);
    const long long total = (long long)a.n_frames * a.slots;
    const int blocks = (int)(total < 8192 ? total : 8192);
    hipLaunchKernelGGL(flow_track_kernel, dim3(blocks), dim3(64), (size_t)8 * side * side * sizeof(float), stream, a);
}

}  // namespace ocvar
