// flow_emul.cpp -- host build of the flow tracking core (opencv-ar_amd/csrc/flow_core.h) for the flow tests: the sequential
// references flow_pyramid_level, flow_track_corner and flow_track_frame, which the kernels of flow.hip must match byte for byte.
#include "flow_core.h"
#include <vector>

using namespace ocvar;

extern "C" {

// The layout of a W x H frame's pyramid: dims = L, w[6], h[6], pitch[6] (19 ints); offs = off[6], bytes (7 long longs).
void flow_geom_emul(int W, int H, int half_win, int levels, int* dims, long long* offs) {
    const FlowGeom g = flow_geom(W, H, half_win, levels);
    dims[0] = g.L;
    for (int l = 0; l <= FLOW_MAX_LEVELS; l++) {
        dims[1 + l] = g.w[l];
        dims[7 + l] = g.h[l];
        dims[13 + l] = g.pitch[l];
        offs[l] = g.off[l];
    }
    offs[6] = g.bytes;
}

void flow_grey_level_emul(const uint8_t* frame, int W, int H, long long row_stride, int fmt, uint8_t* dst, int dst_pitch) {
    flow_grey_level(frame, W, H, row_stride, fmt, dst, dst_pitch);
}

void flow_pyramid_level_emul(const uint8_t* src, int W, int H, int src_pitch, uint8_t* dst, int dst_pitch) {
    flow_pyramid_level(src, W, H, src_pitch, dst, dst_pitch);
}

// Levels 0 .. L of one frame into pyr (flow_geom's bytes).
void flow_build_pyramid_emul(const uint8_t* frame, int W, int H, long long row_stride, int fmt, int half_win, int levels, uint8_t* pyr) {
    flow_build_pyramid(frame, row_stride, fmt, flow_geom(W, H, half_win, levels), pyr);
}

// One frame pair in format fmt: the record slots of `in` under `count` into `out` (which may be `in`), status [slots] and err
// [slots][4] (either may be null).  Returns the number of records tracked.
int flow_track_frame_emul(const uint8_t* prev, long long prev_row_stride, const uint8_t* next, long long next_row_stride, int W, int H, int fmt,
                          const OcvarFlowParams* params, const CameraRec* cam, const MarkerRec* in, int count, int slots, MarkerRec* out,
                          int* status, float* err) {
    const FlowGeom g = flow_geom(W, H, params->half_win, params->levels);
    std::vector<uint8_t> A((size_t)g.bytes), B((size_t)g.bytes);
    flow_build_pyramid(prev, prev_row_stride, fmt, g, A.data());
    flow_build_pyramid(next, next_row_stride, fmt, g, B.data());
    return flow_track_frame(A.data(), B.data(), g, flow_args_make(*params), *cam, in, count, slots, out, status, err);
}

// n points pts [n][2] float32 from the grey W x H image prev to next (rows W bytes apart): out [n][2], codes [n], err [n].
void flow_track_points_emul(const uint8_t* prev, const uint8_t* next, int W, int H, const OcvarFlowParams* params, const float* pts, int n,
                            float* out, int* codes, float* err) {
    const FlowGeom g = flow_geom(W, H, params->half_win, params->levels);
    std::vector<uint8_t> A((size_t)g.bytes), B((size_t)g.bytes);
    flow_build_pyramid(prev, W, OCVAR_FMT_GRAY, g, A.data());
    flow_build_pyramid(next, W, OCVAR_FMT_GRAY, g, B.data());
    std::vector<float> I(FLOW_MAX_SIDE * FLOW_MAX_SIDE), J(FLOW_MAX_SIDE * FLOW_MAX_SIDE);
    const FlowArgs fa = flow_args_make(*params);
    for (int i = 0; i < n; i++)
        codes[i] = flow_track_corner(A.data(), B.data(), g, fa, pts[2 * i], pts[2 * i + 1], I.data(), J.data(), out + 2 * i, out + 2 * i + 1, err + i);
}

}  // extern "C"
