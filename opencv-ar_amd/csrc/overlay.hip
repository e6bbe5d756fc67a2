// overlay.hip -- opt-in drawing of overlay images onto the markers of device-resident frames (ocvar_hip_render /
// ocvar_hip_render_records).  The definition is overlay_core.h's; its host build (tests/emul/overlay_emul.cpp) gives these
// kernels' bytes.  Two launches per chunk of frames: overlay_setup_kernel (one lane per record: map, overlay, box) and
// overlay_draw_kernel (by frame tile, so that overlapping markers neither race nor change their order).
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

// One lane per (frame, record slot): the record's OverlayDraw and OverlayBox; slots past the frame's count get an empty box.
__global__ __launch_bounds__(256) void overlay_setup_kernel(OverlayArgs oa, const MarkerRec* recs, const int* counts, int stride,
                                                           int n_frames, int W, int H) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_frames * stride) return;
    const int f = (int)(i / stride), k = (int)(i - (long long)f * stride);
    int n = counts[f];
    n = n < stride ? n : stride;
    OverlayDraw d;
    OverlayBox b;
    if (k < n) {
        overlay_setup(recs[i], *oa.table, W, H, d, b);
    } else {
        b.x0 = 1; b.y0 = 1; b.x1 = 0; b.y1 = 0;
        d = OverlayDraw{};
        d.slot = -1;
    }
    oa.draws[i] = d;
    oa.boxes[i] = b;
}

constexpr int OVL_LANE_PX = 4;                   // consecutive pixels of a row a lane owns: 4, 12 or 16 bytes, whole dwords
constexpr int OVL_TILE_W = 64 * OVL_LANE_PX;     // columns of a wave's (and a workgroup's) tile
constexpr int OVL_WAVE_ROWS = 4;                 // consecutive rows a wave owns
constexpr int OVL_WAVES = 4;
constexpr int OVL_TILE_H = OVL_WAVES * OVL_WAVE_ROWS;

template <int BPP>
OCVAR_D void ovl_put(unsigned* q, int byte, unsigned v) {
    const int s = 8 * (byte & 3);
    q[byte >> 2] = (q[byte >> 2] & ~(255u << s)) | (v << s);
}

// A workgroup owns a tile of OVL_TILE_W x OVL_TILE_H pixels of one frame, a wave OVL_WAVE_ROWS rows of it, a lane OVL_LANE_PX
// consecutive pixels of each of those rows.  The wave walks the frame's record slots 64 at a time: every lane tests one box
// against the wave's rows, the ballot is the list of records to draw, in output order, and a wave none of whose ballots has a
// bit returns without having loaded a pixel byte.  A row's pixels are loaded once, when the first record covers one of them
// with alpha > 0, blended in registers record after record, and stored once.  ALIGNED (the frames' address and both strides
// are multiples of 4): a lane's pixels are BPP whole dwords, loaded and stored as such, except the lane that crosses the row's
// end; everything else goes byte by byte, and only the bytes of pixels that changed are written (colour bytes alone).
template <int FMT, bool ALIGNED>
__global__ __launch_bounds__(64 * OVL_WAVES) void overlay_draw_kernel(OverlayArgs oa, uint8_t* frames, int W, int H, long long row_stride,
                                                                      long long frame_stride, int stride) {
    constexpr int BPP = (FMT == OCVAR_FMT_GRAY) ? 1 : ((FMT == OCVAR_FMT_BGR || FMT == OCVAR_FMT_RGB) ? 3 : 4);
    constexpr int NC = BPP == 1 ? 1 : 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.z;
    const int tx0 = blockIdx.x * OVL_TILE_W, tx1 = min(tx0 + OVL_TILE_W, W) - 1;
    const int wy0 = blockIdx.y * OVL_TILE_H + wave * OVL_WAVE_ROWS, wy1 = min(wy0 + OVL_WAVE_ROWS, H) - 1;
    if (wy0 >= H) return;
    const OverlayBox* boxes = oa.boxes + (size_t)f * stride;
    const OverlayDraw* draws = oa.draws + (size_t)f * stride;
    bool any = false;
    for (int base = 0; base < stride; base += 64) {
        const int k = base + lane;
        bool hit = false;
        if (k < stride) {
            const OverlayBox b = boxes[k];
            hit = b.x0 <= tx1 && b.x1 >= tx0 && b.y0 <= wy1 && b.y1 >= wy0;
        }
        any = any || __ballot(hit) != 0ull;
    }
    if (!any) return;
    const int x = tx0 + OVL_LANE_PX * lane;
    uint8_t* frame = frames + (size_t)f * frame_stride;
    for (int y = wy0; y <= wy1; y++) {
        unsigned q[BPP];
        bool loaded = false;
        unsigned dirty = 0;
        uint8_t* p = frame + (long long)y * row_stride + (long long)x * BPP;
        const bool whole = ALIGNED && x + OVL_LANE_PX <= W;
        for (int base = 0; base < stride; base += 64) {
            const int kl = base + lane;
            bool hit = false;
            if (kl < stride) {
                const OverlayBox b = boxes[kl];
                hit = b.x0 <= tx1 && b.x1 >= tx0 && b.y0 <= y && b.y1 >= y;
            }
            unsigned long long todo = __ballot(hit);
            while (todo) {   // (uniform)
                const int k = base + __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const OverlayBox b = boxes[k];
                if (x > b.x1 || x + OVL_LANE_PX - 1 < b.x0) continue;
                const OverlayDraw d = draws[k];
                const OverlayTex tex = oa.table->tex[d.slot];
                unsigned c[OVL_LANE_PX];
                unsigned alpha = 0;
                OCVAR_UNROLL
                for (int i = 0; i < OVL_LANE_PX; i++) {
                    c[i] = 0;
                    int U, V;
                    if (x + i >= b.x0 && x + i <= b.x1 && overlay_coords(d.m, x + i, y, tex.w, tex.h, &U, &V)) c[i] = overlay_sample(tex, U, V);
                    alpha |= c[i] >> 24;
                }
                if (!alpha) continue;
                if (!loaded) {
                    loaded = true;
                    OCVAR_UNROLL
                    for (int j = 0; j < BPP; j++) q[j] = 0;
                    if (whole) {
                        const unsigned* pw = reinterpret_cast<const unsigned*>(p);
                        OCVAR_UNROLL
                        for (int j = 0; j < BPP; j++) q[j] = pw[j];
                    } else {
                        OCVAR_UNROLL
                        for (int i = 0; i < OVL_LANE_PX; i++)
                            if (x + i < W) {
                                OCVAR_UNROLL
                                for (int j = 0; j < NC; j++) ovl_put<BPP>(q, i * BPP + j, p[i * BPP + j]);
                            }
                    }
                }
                OCVAR_UNROLL
                for (int i = 0; i < OVL_LANE_PX; i++)
                    if (c[i] >> 24) {   // (a covered pixel lies in the record's box, and the box in the frame)
                        unsigned v[3] = {(unsigned)run_byte(q, i * BPP), NC > 1 ? (unsigned)run_byte(q, i * BPP + NC - 2) : 0u,
                                         NC > 1 ? (unsigned)run_byte(q, i * BPP + NC - 1) : 0u};
                        overlay_blend_px(FMT, c[i], v);
                        OCVAR_UNROLL
                        for (int j = 0; j < NC; j++) ovl_put<BPP>(q, i * BPP + j, v[j]);
                        dirty |= 1u << i;
                    }
            }
        }
        if (!dirty) continue;
        if (whole) {
            unsigned* pw = reinterpret_cast<unsigned*>(p);
            OCVAR_UNROLL
            for (int j = 0; j < BPP; j++) pw[j] = q[j];
        } else {
            OCVAR_UNROLL
            for (int i = 0; i < OVL_LANE_PX; i++)
                if ((dirty >> i) & 1u) {
                    OCVAR_UNROLL
                    for (int j = 0; j < NC; j++) p[i * BPP + j] = (uint8_t)run_byte(q, i * BPP + j);
                }
        }
    }
}

template <int FMT>
static void launch_draw(const OverlayArgs& oa, uint8_t* frames, int W, int H, long long row_stride, long long frame_stride, int n_frames,
                        int stride, bool aligned, hipStream_t stream) {
    const dim3 grid((W + OVL_TILE_W - 1) / OVL_TILE_W, (H + OVL_TILE_H - 1) / OVL_TILE_H, n_frames);
    if (aligned)
        hipLaunchKernelGGL((overlay_draw_kernel<FMT, true>), grid, dim3(64 * OVL_WAVES), 0, stream, oa, frames, W, H, row_stride, frame_stride, stride);
    else
        hipLaunchKernelGGL((overlay_draw_kernel<FMT, false>), grid, dim3(64 * OVL_WAVES), 0, stream, oa, frames, W, H, row_stride, frame_stride, stride);
}

void launch_overlay(const OverlayArgs& oa, uint8_t* frames, int W, int H, long long row_stride, long long frame_stride, int n_frames,
                    int format, const MarkerRec* recs, const int* counts, int stride, hipStream_t stream) {
    if (n_frames <= 0 || stride <= 0) return;
    const long long lanes = (long long)n_frames * stride;
    hipLaunchKernelGGL(overlay_setup_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, oa, recs, counts, stride, n_frames, W, H);
    const bool aligned = frames_dwords(frames, row_stride, frame_stride);
    switch (format) {
        case OCVAR_FMT_BGR: launch_draw<OCVAR_FMT_BGR>(oa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
        case OCVAR_FMT_RGB: launch_draw<OCVAR_FMT_RGB>(oa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
        case OCVAR_FMT_BGRA: launch_draw<OCVAR_FMT_BGRA>(oa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
        case OCVAR_FMT_RGBA: launch_draw<OCVAR_FMT_RGBA>(oa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
        default: launch_draw<OCVAR_FMT_GRAY>(oa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
    }
}

}  // namespace ocvar
