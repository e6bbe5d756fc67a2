// annotate_emul.cpp -- host build of the annotation core (opencv-ar_amd/csrc/annotate_core.h) for the annotate tests: the
// sequential reference annotate_frame, which the kernels of annotate.hip must match byte for byte, the setup of one record, the
// style validator and the tables.  With -DANNOTATE_EMUL_MAIN it is a stand-alone program for the sanitizers.
#include "annotate_core.h"
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace ocvar;

extern "C" {

// One frame under its records; returns the number of records that drew.
int annotate_frame_emul(uint8_t* frame, int W, int H, long long row_stride, int fmt, const MarkerRec* recs, int count, int stride,
                        const OcvarAnnotateStyle* st, const CameraRec* cam) {
    return annotate_frame(frame, W, H, row_stride, fmt, recs, count, stride, *st, *cam);
}

// The primitives of one record (AnnoRec, 680 bytes) and its box (4 ints); returns 1 if it draws.
int annotate_setup_emul(const MarkerRec* rec, const OcvarAnnotateStyle* st, const CameraRec* cam, int W, int H, AnnoRec* out, int* box) {
    AnnoBox b;
    const bool ok = anno_setup(*rec, *st, *cam, W, H, *out, b);
    box[0] = b.x0; box[1] = b.y0; box[2] = b.x1; box[3] = b.y1;
    return ok ? 1 : 0;
}

int annotate_style_bad_emul(const OcvarAnnotateStyle* st, int have_camera) { return anno_style_bad(st, have_camera != 0); }
void annotate_default_style_emul(OcvarAnnotateStyle* st) { anno_default_style(st); }
unsigned long long annotate_glyph_emul(int d) { return anno_glyph(d); }
unsigned annotate_palette_emul(int t) { return anno_palette(t); }
int annotate_style_size_emul() { return (int)sizeof(OcvarAnnotateStyle); }

}  // extern "C"

#ifdef ANNOTATE_EMUL_MAIN
// Frames 1x1, 3x2, 257x17 and 70x37 in every format, each in a buffer of exactly its size (the sanitizer sees any byte beyond
// it); records at, on and beyond every edge, thickness 16 at a corner, coordinates at and beyond the clamp range, poses that put
// points behind the camera.  Prints the number of pixels changed.
static MarkerRec rec_of(const float* sq, int tid, double score) {
    MarkerRec r;
    std::memset(&r, 0, sizeof r);
    for (int i = 0; i < 8; i++) r.square[i] = sq[i];
    r.templateId = tid;
    r.score = score;
    r.aspectRatio = 1.0;
    const double R[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1}, t[3] = {0.1, -0.1, 6.0};
    gl_from_pose(R, t, r.glMatrix);
    return r;
}

int main() {
    const int sizes[4][2] = {{1, 1}, {3, 2}, {257, 17}, {70, 37}};
    CameraRec cam;
    std::memset(&cam, 0, sizeof cam);
    long long changed = 0;
    for (int si = 0; si < 4; si++)
        for (int fmt = 0; fmt < 5; fmt++)
            for (int th = 1; th <= 16; th += 15)
                for (int dist = 0; dist < 2; dist++) {
                    const int W = sizes[si][0], H = sizes[si][1], bpp = overlay_bpp(fmt);
                    cam.width = W;
                    cam.height = H;
                    cam.cameraMatrix[0] = cam.cameraMatrix[4] = 0.9 * W;
                    cam.cameraMatrix[2] = 0.5 * W;
                    cam.cameraMatrix[5] = 0.5 * H;
                    cam.cameraMatrix[8] = 1;
                    cam.distCoeffs[0] = dist ? -0.2 : 0.0;
                    cam.distCoeffs[2] = dist ? 0.01 : 0.0;
                    const float w = (float)W, h = (float)H, big = 3.0e6f, huge = 3.0e38f;
                    const float quads[][8] = {
                        {0, 0, w - 1, 0, w - 1, h - 1, 0, h - 1},                       // on every edge
                        {-8, -8, w + 7, -8, w + 7, h + 7, -8, h + 7},                   // just beyond every edge
                        {-0.5f, -0.5f, w - 0.5f, -0.5f, w - 0.5f, h - 0.5f, -0.5f, h - 0.5f},   // at the pixels' outer borders
                        {w - 1, h - 1, w + 20, h - 1, w + 20, h + 20, w - 1, h + 20},   // corner 0 on the last pixel
                        {-30, -30, -10, -30, -10, -10, -30, -10},                        // wholly outside
                        {-big, -big, big, -big, big, big, -big, big},                   // beyond the clamp range on every side
                        {-huge, 0.5f * h, huge, 0.5f * h, huge, huge, -huge, -huge},    // the largest floats
                        {1048576.f, 1048576.f, -1048576.f, 1048576.f, 0, 0, w, h},      // at the clamp range
                        {0.25f * w, 0.25f * h, 0.75f * w, 0.75f * h, 0.75f * w, 0.25f * h, 0.25f * w, 0.75f * h},   // a bow-tie
                        {0.5f * w, 0.5f * h, 0.5f * w, 0.5f * h, 0.5f * w, 0.5f * h, 0.5f * w, 0.5f * h},           // a point
                        {std::numeric_limits<float>::quiet_NaN(), 0, 1, 0, 1, 1, 0, 1},
                        {std::numeric_limits<float>::infinity(), 0, 1, 0, 1, 1, 0, 1}};
                    const int nq = (int)(sizeof quads / sizeof quads[0]);
                    std::vector<MarkerRec> recs;
                    for (int k = 0; k < nq; k++) recs.push_back(rec_of(quads[k], k == 1 ? 4095 : (k == 2 ? 2147483647 : k), k == 3 ? 0.0 : 1.0));
                    recs[4].templateId = -7;
                    recs[5].glMatrix[14] = 3.0;                                           // the marker behind the camera
                    recs[6].glMatrix[14] = -0.5;                                          // the camera inside the cube
                    recs[7].glMatrix[3] = std::numeric_limits<double>::quiet_NaN();
                    recs[8].glMatrix[12] = 1e300;
                    OcvarAnnotateStyle st;
                    anno_default_style(&st);
                    st.flags = ANNO_FLAGS;
                    st.thickness = th;
                    st.label_scale = th == 1 ? 0 : 8;
                    st.axis_length = th == 1 ? 1.0 : 1e9;
                    st.cube_height = th == 1 ? 7.0 : 0.0;
                    st.outline[3] = 128;
                    if (anno_style_bad(&st, true)) return 2;
                    const size_t row = (size_t)W * bpp, bytes = row * H;
                    std::vector<uint8_t> frame(bytes, 100), before(frame);
                    const int drawn = annotate_frame(frame.data(), W, H, (long long)row, fmt, recs.data(), nq + 5, nq, st, cam);
                    if (drawn < 3) return 3;
                    for (size_t i = 0; i < bytes; i++) changed += frame[i] != before[i];
                }
    std::printf("annotate_emul: %lld bytes changed\n", changed);
    return changed > 0 ? 0 : 1;
}
#endif
