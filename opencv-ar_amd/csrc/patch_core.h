// patch_core.h -- the rectified image of every marker a frame's records hold, cut out of frames that stay in device memory
// (opt-in: ocvar_hip_patches / ocvar_hip_patches_records).  The reference's public cvarInvertPerspective(frame, patch,
// record.square, cvarSquare(pw, ph, ccw = 0)) (opencvar.cpp:510-516: cvGetPerspectiveTransform + cvWarpPerspective), with the
// arithmetic decode_core.h already has for the code readout and nothing beyond it.
//
// For one record with square s (8 floats) and a patch of pw x ph pixels (2 .. OCVAR_MAX_PATCH_SIDE each way):
//   map      m32 = perspective_from_quad(s, pw, ph), M = invert_map(m32): record corners 0, 1, 2, 3 land on patch pixels (0, 0),
//            (pw-1, 0), (pw-1, ph-1), (0, ph-1).
//   pixel    byte c of patch pixel (x, y) is warp_sample_px(px_c, W, H, M, x, y), px_c(ix, iy) = byte c of frame pixel (ix, iy)
//            of the W x H frame; outside the frame reads 0.  Every byte of a pixel is warped alike, as cvWarpPerspective does:
//            the patch has the frame format's bytes per pixel (1, 3 or 4) in the frame's memory order, and byte 3 of a
//            four-channel pixel is warped like the others.
//   status   slot k of a frame is written (status 1) when k < min(count, slots), all eight coordinates are finite and at most
//            OCVAR_PATCH_MAX_COORD in magnitude (tested before any arithmetic: it keeps every cast defined),
//            perspective_from_quad succeeds and, with OCVAR_PATCH_MATCHED_ONLY, score > 0.  Every other slot gets status 0 and
//            none of its patch bytes is touched.  A written patch that lies wholly outside the frame is all zeros, status 1.
//            Quads that are not convex give whatever the formulas give.
//   flip     OCVAR_PATCH_FLIP_ROWS stores patch row r at row ph-1-r and changes nothing else: templates are loaded flipped
//            vertically (see ocvar_hip_set_board), so with the flag the patch reads like the template's image file.
// Patches are [slots][ph][pw][bpp] bytes, contiguous; statuses [slots] ints (may be absent).
//
// All arithmetic is integer or IEEE double (-ffp-contract=off): the host build (tests/emul/patch_emul.cpp) gives the bytes of
// the kernel (patch.hip).  patch_extract_frame is that host reference, sequential.
#pragma once
#include "hd.h"
#include "frames_core.h"
#include "ocvar_hip.h"
#include "decode_core.h"
#include "tail_core.h"
#include <math.h>

namespace ocvar {

constexpr int PATCH_MAX_SIDE = OCVAR_MAX_PATCH_SIDE;
constexpr float PATCH_MAX_COORD = 1e6f;   // OCVAR_PATCH_MAX_COORD
constexpr int PATCH_FLAGS = OCVAR_PATCH_FLIP_ROWS | OCVAR_PATCH_MATCHED_ONLY;

// The status rule for a record inside its frame's count, and the record's map M (patch pixels -> frame pixels); false: the
// slot is not written.
OCVAR_HD bool patch_map(const MarkerRec& r, int pw, int ph, int flags, double* M) {
    for (int i = 0; i < 8; i++)
        if (!(fabsf(r.square[i]) <= PATCH_MAX_COORD)) return false;   // (a NaN fails the comparison too)
    if ((flags & OCVAR_PATCH_MATCHED_ONLY) && !(r.score > 0.0)) return false;
    float m32[9];
    if (!perspective_from_quad(r.square, pw, ph, m32)) return false;
    invert_map(m32, M);
    return true;
}

// Byte c of patch pixel (x, y) from a W x H frame of bpp bytes per pixel, rows row_stride bytes apart.
OCVAR_HD int patch_sample(const uint8_t* frame, int W, int H, long long row_stride, int bpp, int c, const double* M, int x, int y) {
    return warp_sample_px([=](int ix, int iy) -> int { return frame[(long long)iy * row_stride + (long long)ix * bpp + c]; }, W, H, M, x, y);
}

// The host reference: the `slots` patch slots and statuses of one W x H frame in format fmt under its records
// recs[0 .. min(count, slots) - 1], sequentially.  status may be nullptr.  Returns the number of slots written.
inline int patch_extract_frame(const uint8_t* frame, int W, int H, long long row_stride, int fmt, const MarkerRec* recs, int count, int slots,
                               uint8_t* patches, int pw, int ph, int flags, int* status) {
    const int bpp = format_bpp(fmt), n = count < slots ? count : slots;
    int written = 0;
    for (int k = 0; k < slots; k++) {
        double M[9];
        const bool ok = k < n && patch_map(recs[k], pw, ph, flags, M);
        if (status) status[k] = ok ? 1 : 0;
        if (!ok) continue;
        written++;
        uint8_t* out = patches + (size_t)k * ph * pw * bpp;
        for (int y = 0; y < ph; y++) {
            const int row = (flags & OCVAR_PATCH_FLIP_ROWS) ? ph - 1 - y : y;
            for (int x = 0; x < pw; x++)
                for (int c = 0; c < bpp; c++)
                    out[((size_t)row * pw + x) * bpp + c] = (uint8_t)patch_sample(frame, W, H, row_stride, bpp, c, M, x, y);
        }
    }
    return written;
}

}  // namespace ocvar
