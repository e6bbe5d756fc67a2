// overlay_emul.cpp -- host build of the overlay core (opencv-ar_amd/csrc/overlay_core.h) for the overlay tests: the sequential
// reference overlay_render_frame, which the kernels of overlay.hip must match byte for byte.
#include "overlay_core.h"
#include <memory>

using namespace ocvar;

extern "C" {

// One frame under its records.  The n overlays: tight RGBA images tex[i] of tex_w[i] x tex_h[i] texels for template tids[i]
// (-1: the default overlay).  Returns the number of records that drew.
int overlay_render_frame_emul(uint8_t* frame, int W, int H, long long row_stride, int fmt, const MarkerRec* recs, int count, int stride,
                              const uint8_t* const* tex, const int* tex_w, const int* tex_h, const int* tids, int n) {
    std::unique_ptr<OverlayTable> tab(new OverlayTable());
    for (auto& t : tab->tex) t = OverlayTex{nullptr, 0, 0};
    tab->dflt = -1;
    for (auto& m : tab->map) m = -1;
    for (int i = 0; i < n && i < OVL_MAX; i++) {
        tab->tex[i] = OverlayTex{reinterpret_cast<const uint32_t*>(tex[i]), tex_w[i], tex_h[i]};
        if (tids[i] < 0) tab->dflt = i;
        else if (tids[i] < OCVAR_MAX_TEMPLATES) tab->map[tids[i]] = i;
    }
    return overlay_render_frame(frame, W, H, row_stride, fmt, recs, count, stride, *tab);
}

// the grey the library gives a B G R pixel (hd.h), as the overlay core restates it
int overlay_grey_emul(int b, int g, int r) {
    unsigned d[1] = {0};
    overlay_blend_px(OCVAR_FMT_GRAY, (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16) | (255u << 24), d);
    return (int)d[0];
}

}  // extern "C"
