// annotate.hip -- opt-in stroking of outlines, corner dots, pose cubes and axes and template ids onto the markers of
// device-resident frames (ocvar_hip_annotate / ocvar_hip_annotate_records).  The definition is annotate_core.h's; its host build
// (tests/emul/annotate_emul.cpp) gives these kernels' bytes.  Two launches per chunk of frames: annotate_setup_kernel (one lane
// per record slot: its primitives and boxes) and annotate_draw_kernel (by frame tile, as overlay.hip draws, so that overlapping
// records neither race nor change their order).
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

// One lane per (frame, record slot): the slot's AnnoRec and AnnoBox; slots past the frame's count get an empty box.
__global__ __launch_bounds__(256) void annotate_setup_kernel(AnnoArgs aa, const MarkerRec* recs, const int* counts, int stride, int n_frames,
                                                            int W, int H, OcvarAnnotateStyle st, CameraRec cam) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_frames * stride) return;
    const int f = (int)(i / stride), k = (int)(i - (long long)f * stride);
    int n = counts[f];
    n = n < stride ? n : stride;
    AnnoBox b;
    anno_box_empty(b);
    if (k < n) anno_setup(recs[i], st, cam, W, H, aa.recs[i], b);   // (a slot with an empty box is never read)
    aa.boxes[i] = b;
}

constexpr int ANNO_LANE_PX = 4;                   // consecutive pixels of a row a lane owns: 4, 12 or 16 bytes, whole dwords
constexpr int ANNO_TILE_W = 64 * ANNO_LANE_PX;    // columns of a wave's (and a workgroup's) tile
constexpr int ANNO_WAVE_ROWS = 4;                 // consecutive rows a wave owns
constexpr int ANNO_WAVES = 4;
constexpr int ANNO_TILE_H = ANNO_WAVES * ANNO_WAVE_ROWS;

OCVAR_D void anno_put(unsigned* q, int byte, unsigned v) {
    const int s = 8 * (byte & 3);
    q[byte >> 2] = (q[byte >> 2] & ~(255u << s)) | (v << s);
}

// The columns of row y a stroke can reach, conservatively: a covered pixel is within the radius of a point of the spine, so that
// point lies in the band of rows y -+ radius, and the pixel within the radius of the spine's columns there.  float32 on values
// below 2^25 is good to well under a pixel; the span is widened by two.  false: the spine does not meet the band.  (Wave-uniform:
// it culls before any per-pixel arithmetic and never decides coverage -- anno_seg_covers does.)
OCVAR_D bool anno_row_span(const AnnoSeg& s, int y, int* lo, int* hi) {
    const int py = 16 * y, ylo = py - s.r, yhi = py + s.r;
    if (max(s.ay, s.by) < ylo || min(s.ay, s.by) > yhi) return false;
    float xa = (float)s.ax, xb = (float)s.bx;
    const int dy = s.by - s.ay;
    if (dy != 0) {
        const float inv = 1.0f / (float)dy;
        float t0 = (float)(ylo - s.ay) * inv, t1 = (float)(yhi - s.ay) * inv;
        if (t0 > t1) {
            const float t = t0;
            t0 = t1;
            t1 = t;
        }
        t0 = fminf(fmaxf(t0, 0.0f), 1.0f);
        t1 = fminf(fmaxf(t1, 0.0f), 1.0f);
        const float dx = xb - xa;
        xb = xa + dx * t1;
        xa = xa + dx * t0;
    }
    const float r = (float)s.r;
    *lo = (int)floorf((fminf(xa, xb) - r) * 0.0625f) - 2;
    *hi = (int)ceilf((fmaxf(xa, xb) + r) * 0.0625f) + 2;
    return true;
}

// A workgroup owns a tile of ANNO_TILE_W x ANNO_TILE_H pixels of one frame, a wave ANNO_WAVE_ROWS rows of it, a lane ANNO_LANE_PX
// consecutive pixels of each of those rows -- overlay.hip's scheme: the wave walks the frame's record slots 64 at a time, every
// lane tests one record's box against the wave's rows, the ballot is the list of records to draw, in output order, and a wave
// none of whose ballots has a bit ends without having loaded a pixel byte.
// A stroke covers a sliver of its record's box, so a record on the list is culled primitive by primitive before any per-pixel
// arithmetic.  Wave-uniform: the record's word of live primitives, each live primitive's own grown box against the wave's rows
// and the tile's columns (its 32 bytes are read once for all the wave's rows), then per row the box's rows and the columns the
// stroke can reach in that row (anno_row_span).  Per lane: its four pixels against those columns.  Only a lane that passes runs
// anno_seg_covers.  A row's pixels are loaded once, when the first record covers one of them with alpha > 0, blended in registers
// record after record, and stored once.  ALIGNED (the frames' address and both strides are multiples of 4): a lane's pixels are
// BPP whole dwords, loaded and stored as such, except the lane that crosses the row's end; everything else goes byte by byte, and
// only the colour bytes of pixels that changed are written.
template <int FMT, bool ALIGNED>
__global__ __launch_bounds__(64 * ANNO_WAVES) void annotate_draw_kernel(AnnoArgs aa, uint8_t* frames, int W, int H, long long row_stride,
                                                                        long long frame_stride, int stride) {
    constexpr int BPP = (FMT == OCVAR_FMT_GRAY) ? 1 : ((FMT == OCVAR_FMT_BGR || FMT == OCVAR_FMT_RGB) ? 3 : 4);
    constexpr int NC = BPP == 1 ? 1 : 3;
    constexpr int ROWS = ANNO_WAVE_ROWS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.z;
    const int tx0 = blockIdx.x * ANNO_TILE_W, tx1 = min(tx0 + ANNO_TILE_W, W) - 1;
    const int wy0 = blockIdx.y * ANNO_TILE_H + wave * ROWS, wy1 = min(wy0 + ROWS, H) - 1;
    if (wy0 >= H) return;
    const AnnoBox* boxes = aa.boxes + (size_t)f * stride;
    const AnnoRec* recs = aa.recs + (size_t)f * stride;
    const int x = tx0 + ANNO_LANE_PX * lane;
    const bool whole = ALIGNED && x + ANNO_LANE_PX <= W;
    uint8_t* const p0 = frames + (size_t)f * frame_stride + (long long)wy0 * row_stride + (long long)x * BPP;
    unsigned q[ROWS][BPP];
    unsigned loaded = 0, dirty = 0;   // bit r: row r's pixels are in q; bit 4 r + i: pixel i of row r changed
    for (int base = 0; base < stride; base += 64) {
        const int kl = base + lane;
        bool hit = false;
        if (kl < stride) {
            const AnnoBox b = boxes[kl];
            hit = b.x0 <= tx1 && b.x1 >= tx0 && b.y0 <= wy1 && b.y1 >= wy0;
        }
        unsigned long long todo = __ballot(hit);
        while (todo) {   // (uniform)
            const int k = base + __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const AnnoRec* a = recs + k;
            unsigned live = boxes[k].live;
            unsigned c[ROWS][ANNO_LANE_PX];
            OCVAR_UNROLL
            for (int r = 0; r < ROWS; r++) {
                OCVAR_UNROLL
                for (int i = 0; i < ANNO_LANE_PX; i++) c[r][i] = 0;
            }
            const bool label = (live >> ANNO_SEGS) & 1u;
            live &= (1u << ANNO_SEGS) - 1u;
            while (live) {   // (uniform)
                const int pr = __ffs((int)live) - 1;
                live &= live - 1u;
                const AnnoSeg s = a->seg[pr];
                if (s.y0 > wy1 || s.y1 < wy0 || s.x0 > tx1 || s.x1 < tx0) continue;   // (uniform)
                OCVAR_UNROLL
                for (int r = 0; r < ROWS; r++) {
                    const int y = wy0 + r;
                    int lo, hi;
                    if (y < s.y0 || y > s.y1 || !anno_row_span(s, y, &lo, &hi)) continue;   // (uniform)
                    lo = max(lo, (int)s.x0);
                    hi = min(hi, (int)s.x1);
                    if (x > hi || x + ANNO_LANE_PX - 1 < lo) continue;
                    OCVAR_UNROLL
                    for (int i = 0; i < ANNO_LANE_PX; i++)
                        if (x + i >= lo && x + i <= hi && anno_seg_covers(s, x + i, y)) c[r][i] = s.rgba;
                }
            }
            if (label && a->y0 <= wy1 && a->y1 >= wy0 && a->x0 <= tx1 && a->x1 >= tx0) {   // (uniform)
                const int lx0 = a->x0, lx1 = a->x1, ly0 = a->y0, ly1 = a->y1;
                const unsigned lc = a->rgba;
                if (x <= lx1 && x + ANNO_LANE_PX - 1 >= lx0) {
                    OCVAR_UNROLL
                    for (int r = 0; r < ROWS; r++) {
                        const int y = wy0 + r;
                        if (y < ly0 || y > ly1) continue;
                        OCVAR_UNROLL
                        for (int i = 0; i < ANNO_LANE_PX; i++)
                            if (x + i >= lx0 && x + i <= lx1 && anno_label_covers(*a, x + i, y)) c[r][i] = lc;
                    }
                }
            }
            OCVAR_UNROLL
            for (int r = 0; r < ROWS; r++) {
                unsigned alpha = 0;
                OCVAR_UNROLL
                for (int i = 0; i < ANNO_LANE_PX; i++) alpha |= c[r][i] >> 24;
                if (!alpha) continue;   // (a covered pixel lies in its primitive's box, and the box in the frame: row r exists)
                const uint8_t* p = p0 + (long long)r * row_stride;
                if (!((loaded >> r) & 1u)) {
                    loaded |= 1u << r;
                    OCVAR_UNROLL
                    for (int j = 0; j < BPP; j++) q[r][j] = 0;
                    if (whole) {
                        const unsigned* pw = reinterpret_cast<const unsigned*>(p);
                        OCVAR_UNROLL
                        for (int j = 0; j < BPP; j++) q[r][j] = pw[j];
                    } else {
                        OCVAR_UNROLL
                        for (int i = 0; i < ANNO_LANE_PX; i++)
                            if (x + i < W) {
                                OCVAR_UNROLL
                                for (int j = 0; j < NC; j++) anno_put(q[r], i * BPP + j, p[i * BPP + j]);
                            }
                    }
                }
                OCVAR_UNROLL
                for (int i = 0; i < ANNO_LANE_PX; i++)
                    if (c[r][i] >> 24) {
                        unsigned v[3] = {(unsigned)run_byte(q[r], i * BPP), NC > 1 ? (unsigned)run_byte(q[r], i * BPP + NC - 2) : 0u,
                                         NC > 1 ? (unsigned)run_byte(q[r], i * BPP + NC - 1) : 0u};
                        overlay_blend_px(FMT, c[r][i], v);
                        OCVAR_UNROLL
                        for (int j = 0; j < NC; j++) anno_put(q[r], i * BPP + j, v[j]);
                        dirty |= 1u << (4 * r + i);
                    }
            }
        }
    }
    if (!dirty) return;
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) {
        if (!((dirty >> (4 * r)) & 15u)) continue;
        uint8_t* p = p0 + (long long)r * row_stride;
        if (whole) {
            unsigned* pw = reinterpret_cast<unsigned*>(p);
            OCVAR_UNROLL
            for (int j = 0; j < BPP; j++) pw[j] = q[r][j];
        } else {
            OCVAR_UNROLL
            for (int i = 0; i < ANNO_LANE_PX; i++)
                if ((dirty >> (4 * r + i)) & 1u) {
                    OCVAR_UNROLL
                    for (int j = 0; j < NC; j++) p[i * BPP + j] = (uint8_t)run_byte(q[r], i * BPP + j);
                }
        }
    }
}

template <int FMT>
static void launch_draw(const AnnoArgs& aa, uint8_t* frames, int W, int H, long long row_stride, long long frame_stride, int n_frames,
                        int stride, bool aligned, hipStream_t stream) {
    const dim3 grid((W + ANNO_TILE_W - 1) / ANNO_TILE_W, (H + ANNO_TILE_H - 1) / ANNO_TILE_H, n_frames);
    if (aligned)
        hipLaunchKernelGGL((annotate_draw_kernel<FMT, true>), grid, dim3(64 * ANNO_WAVES), 0, stream, aa, frames, W, H, row_stride, frame_stride, stride);
    else
        hipLaunchKernelGGL((annotate_draw_kernel<FMT, false>), grid, dim3(64 * ANNO_WAVES), 0, stream, aa, frames, W, H, row_stride, frame_stride, stride);
}

void launch_annotate(const AnnoArgs& aa, uint8_t* frames, int W, int H, long long row_stride, long long frame_stride, int n_frames, int format,
                     const MarkerRec* recs, const int* counts, int stride, const OcvarAnnotateStyle& st, const CameraRec& cam,
                     hipStream_t stream) {
    if (n_frames <= 0 || stride <= 0) return;
    const long long lanes = (long long)n_frames * stride;
    hipLaunchKernelGGL(annotate_setup_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, aa, recs, counts, stride, n_frames, W, H,
                       st, cam);
    const bool aligned = frames_dwords(frames, row_stride, frame_stride);
    switch (format) {
        case OCVAR_FMT_BGR: launch_draw<OCVAR_FMT_BGR>(aa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
        case OCVAR_FMT_RGB: launch_draw<OCVAR_FMT_RGB>(aa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
        case OCVAR_FMT_BGRA: launch_draw<OCVAR_FMT_BGRA>(aa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
        case OCVAR_FMT_RGBA: launch_draw<OCVAR_FMT_RGBA>(aa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
        default: launch_draw<OCVAR_FMT_GRAY>(aa, frames, W, H, row_stride, frame_stride, n_frames, stride, aligned, stream); break;
    }
}

}  // namespace ocvar
