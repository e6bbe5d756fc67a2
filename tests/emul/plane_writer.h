// plane_writer.h -- the neighbour plane of a binary image, written straight from the layout's definition (hd.h), for the
// host emulations that read one (bitplane_emul.cpp, follow_emul.cpp).  TEST ONLY.
// With -DOCVAR_NBR_TILED: the product's bit plane (16x14 tiles with a one-pixel apron); without: the raster byte plane.
#pragma once
#include "hd.h"

// the binary image as cvFindContours sees it: the 1-px frame zeroed
inline int emul_bin_at(const uint8_t* bin, int w, int h, int x, int y) {
    if (x < 1 || y < 1 || x > w - 2 || y > h - 2) return 0;
    return bin[(size_t)y * w + x] != 0;
}

// row stride of the plane of an image sw pixels wide
inline int emul_plane_ns(int sw) {
#if defined(OCVAR_NBR_TILED)
    return (sw + 15) & ~15;
#else
    return sw;
#endif
}

// the plane of an sw x sh binary image (ocvar::nbr_plane_bytes(emul_plane_ns(sw), sh) bytes)
inline void emul_make_plane(const uint8_t* bin, int sw, int sh, uint8_t* plane) {
    using namespace ocvar;
    const int ns = emul_plane_ns(sw);
#if defined(OCVAR_NBR_TILED)
    const int ntx = ns / NBR_TILE_W, nty = (sh + NBR_TILE_H - 1) / NBR_TILE_H;
    unsigned* d = reinterpret_cast<unsigned*>(plane);
    for (int ty = 0; ty < nty; ty++)
        for (int tx = 0; tx < ntx; tx++)
            for (int j = 0; j < 16; j++) {
                unsigned v = 0;
                for (int b = 0; b < 18; b++) v |= (unsigned)emul_bin_at(bin, sw, sh, NBR_TILE_W * tx + b - 1, NBR_TILE_H * ty + j - 1) << b;
                d[((size_t)ty * ntx + tx) * 16 + j] = v;
            }
#else
    for (int y = 0; y < sh; y++)
        for (int x = 0; x < ns; x++) {
            unsigned m = 0;
            for (int s = 0; s < 8; s++) m |= (unsigned)emul_bin_at(bin, sw, sh, x + dir_dx(s), y + dir_dy(s)) << s;
            plane[(size_t)y * ns + x] = (uint8_t)m;
        }
#endif
}
