// hd.h -- shared definitions for the HIP kernels (gfx950) of the opencv-ar hot path.
//
// The algorithm cores in *_core.h are written as plain functions so that tests/emul can compile them
// with g++ and check their logic against the oracle without a GPU.  That host build is test-only;
// the product library (libocvar_hip.so) contains the gfx950 code objects and nothing else computes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OCVAR_HD __host__ __device__ __forceinline__
#define OCVAR_D __device__ __forceinline__
#define OCVAR_UNROLL _Pragma("unroll")   // small fixed-size loops over arrays that must become registers (constant indices)
#else
#define OCVAR_HD inline
#define OCVAR_D inline
#define OCVAR_UNROLL
#endif
// OCVAR_OPAQUE(v): the optimiser is to take the per-lane value v as given and not look through it to the expression it came
// from (where it would otherwise compute a variant of that expression again for each use); costs no instruction
#if defined(__HIP_DEVICE_COMPILE__)
#define OCVAR_OPAQUE(v) asm("" : "+v"(v))
#else
#define OCVAR_OPAQUE(v) ((void)0)
#endif

namespace ocvar {

// Pixel-neighbour directions of the border follower, s = 0..7 = E,NE,N,NW,W,SW,S,SE
// (increasing s is counter-clockwise on screen; cvFindContours' icvCodeDeltas order).
OCVAR_HD int dir_dx(int s) { return (s == 0 || s == 1 || s == 7) ? 1 : ((s >= 3 && s <= 5) ? -1 : 0); }
OCVAR_HD int dir_dy(int s) { return (s >= 1 && s <= 3) ? -1 : ((s >= 5 && s <= 7) ? 1 : 0); }

struct Pt { int x, y; };

// BGR2GRAY, (1868 B + 9617 G + 4899 R + 8192) >> 14, as the frame kernel computes it: times four, (7472 B + 38468 G + 19596 R
// + 32768) >> 16, with each coefficient split into a high and a low byte for v_dot4_u32_u8 -- the grey value is byte 2 of
// (dot4(pixel, KH) << 8) + dot4(pixel, KL) + 32768 (the kernel takes it from a 16-bit form of that sum: grey_sum16 below).  One
// word per byte order of the source pixel (B G R x / R G B x); byte 3 is 0, so a four-channel pixel's fourth byte does not
// count.  (tests/test_input_formats_cpu.py checks all 2^24 pixels.)
constexpr unsigned GREY_KH_BGR = 29u | (150u << 8) | (76u << 16), GREY_KL_BGR = 48u | (68u << 8) | (140u << 16);
constexpr unsigned GREY_KH_RGB = 76u | (150u << 8) | (29u << 16), GREY_KL_RGB = 140u | (68u << 8) | (48u << 16);
// c + the sum of the four byte products of a and b (v_dot4_u32_u8)
OCVAR_HD unsigned dot4_u8(unsigned a, unsigned b, unsigned c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int j = 0; j < 4; j++) c += ((a >> (8 * j)) & 255u) * ((b >> (8 * j)) & 255u);
    return c;
#endif
}
// The same grey value as byte 1 of a sum that fits 16 bits, which is how the kernel keeps it (two pixels per register):
// with H = dot4(pixel, KH) (<= 65025) and L = dot4(pixel, KL) (<= 65280), (256 H + L + 32768) >> 16 = (H + ((L + 32768) >> 8)) >> 8
// and (L + 32768) >> 8 = (L >> 8) + 128 exactly, so grey = T >> 8 with T = (H + 128) + (L >> 8) <= 65408.  L >> 8 is byte 1 of L:
// the add picks it itself.  (tests/test_grey_pack_cpu.py: all 2^24 pixels in both byte orders, and the two bounds.)
OCVAR_HD unsigned grey_low16(unsigned pixel, unsigned kl) { return dot4_u8(pixel, kl, 0u); }
OCVAR_HD unsigned grey_sum16(unsigned pixel, unsigned kh, unsigned kl) { return dot4_u8(pixel, kh, 128u) + ((grey_low16(pixel, kl) >> 8) & 255u); }

// The neighbour plane of a binary image (sw x sh, row stride ns: sw rounded up to a multiple of 16).
//
// Host-side test build of the cores: one byte per pixel, raster rows, the 8-neighbour mask (bit s = the neighbour in
// direction s is set); nbr_at() reads it.
//
// Product build (OCVAR_NBR_TILED): a BIT plane with an apron, stored as tiles.  A tile covers 16 columns x 14 rows and is
// 16 dwords (64 bytes, one sector); dword j holds row 14 ty + j - 1, bit b of it column 16 tx + b - 1 (b = 0..17).  So a
// pixel's 3x3 neighbourhood is dwords y % 14 .. y % 14 + 2 of its tile -- one aligned 12-byte load -- at bits x % 16 ..
// x % 16 + 2, and its mask byte follows from those 9 bits (nbr_mask9).  Pixels outside the plane and on cvFindContours'
// zeroed frame are 0.  The tiles of one tile row are contiguous.  0.29 bytes per pixel instead of 1: the binarise kernels
// write it in whole sectors, the followers' dependent loads stay inside one sector for ~10 steps as with byte tiles.
// (A plane is far smaller than 4 GB; offsets are 32-bit and, on the device, built with the 24-bit multiplier: the
// followers compute one per step on a dependent chain.)
constexpr int NBR_TILE_W = 16, NBR_TILE_H = 14, NBR_TILE_BYTES = 64;
OCVAR_HD unsigned umul24(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}
// the low byte of m in all four bytes; v rotated right by s (mod 32) bits -- one instruction each on the device
OCVAR_HD unsigned byte_replicate(unsigned m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(m, m, 0u);
#else
    return (m & 0xffu) * 0x01010101u;
#endif
}
OCVAR_HD unsigned rotate_right(unsigned v, unsigned s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(v, v, s);
#else
    return (v >> (s & 31u)) | (v << ((32u - s) & 31u));
#endif
}
// y / 14 and y % 14 for 0 <= y < 43690 (2^19 / 14 rounded up: exact in that range; images are at most 32767 rows)
OCVAR_HD unsigned div14(unsigned y) { return umul24(y, 37450u) >> 19; }
// bytes of a plane: (ns / 16) tiles per tile row, sh rounded up to whole tile rows
OCVAR_HD long long nbr_plane_bytes(int ns, int sh) {
#if defined(OCVAR_NBR_TILED)
    return (long long)(ns >> 4) * NBR_TILE_BYTES * ((sh + NBR_TILE_H - 1) / NBR_TILE_H);
#else
    return (long long)ns * sh;
#endif
}
// byte offset of tile (tx, ty); of the 3x3 window of pixel (x, y) (dword y % 14 of its tile: rows y-1, y, y+1 follow)
OCVAR_HD unsigned nbr_tile_off(unsigned tx, unsigned ty, int ns) { return (umul24(ty, (unsigned)ns >> 4) + tx) * (unsigned)NBR_TILE_BYTES; }
OCVAR_HD unsigned nbr_win_off(int x, int y, int ns) {
    const unsigned ty = div14((unsigned)y);
    return nbr_tile_off((unsigned)x >> 4, ty, ns) + 4u * ((unsigned)y - 14u * ty);
}
// the same for a packed point x | y << 16 with nt = ns / 16 (the border followers' position format)
OCVAR_HD unsigned nbr_win_off_xy(unsigned xy, unsigned nt) {
    const unsigned y = xy >> 16, ty = div14(y);
    return (umul24(ty, nt) + ((xy >> 4) & 0xfffu)) * (unsigned)NBR_TILE_BYTES + 4u * (y - 14u * ty);
}
// The 8-neighbour mask (E NE N NW W SW S SE = bits 0..7) of the pixel at bit k + 1 of the row words above (a), own (c), below (b).
// (Bit arithmetic instead of a table: on a follower's dependent chain ten VALU operations are shorter than an LDS round trip.)
OCVAR_HD unsigned nbr_mask9(unsigned a, unsigned c, unsigned b, unsigned k) {
    // the row above comes in as NW N NE (bits 0 1 2) and goes to mask bits 3 2 1: a nibble table indexed by the 3 bits
    constexpr unsigned REV = (0u << 0) | (8u << 4) | (4u << 8) | (12u << 12) | (2u << 16) | (10u << 20) | (6u << 24) | (14u << 28);
    const unsigned up = (REV >> (((a >> k) & 7u) << 2)) & 15u;
    const unsigned own = ((c >> (k + 2u)) & 1u) | (((c >> k) & 1u) << 4);
    return up | own | (((b >> k) & 7u) << 5);
}
#if defined(OCVAR_NBR_TILED)
// mask byte of pixel (x, y), 0 <= x < ns, 0 <= y < sh: one 12-byte load
OCVAR_HD unsigned nbr_of(const uint8_t* plane, int x, int y, int ns) {
    const unsigned* w = reinterpret_cast<const unsigned*>(plane + nbr_win_off(x, y, ns));
    return nbr_mask9(w[0], w[1], w[2], (unsigned)x & 15u);
}
// the pixel's own binary value (0 / 1)
OCVAR_HD unsigned nbr_bit(const uint8_t* plane, int x, int y, int ns) {
    const unsigned* w = reinterpret_cast<const unsigned*>(plane + nbr_win_off(x, y, ns));
    return (w[1] >> (((unsigned)x & 15u) + 1u)) & 1u;
}
OCVAR_HD unsigned nbr_at(const uint8_t* plane, int x, int y, int ns) { return nbr_of(plane, x, y, ns); }
#else
OCVAR_HD unsigned nbr_at(const uint8_t* plane, int x, int y, int ns) { return plane[y * ns + x]; }
#endif

// The grey plane is stored in PANELS: panel p of a row holds columns 240 p - 8 .. 240 p + 247 in 256 bytes -- the 256 columns one
// wave of the frame binarise kernel converts (its 240 output columns and the 8-column halo on either side), so that every grey
// store of that kernel is 256 contiguous bytes at a 256-byte boundary: whole 64-byte sectors.  (Stored row-major at the image's
// own pitch, a wave's 240 bytes began at 240 s: five sectors touched, two of them shared with the neighbouring strips' waves; the
// partial sectors made the grey byte the dearest of the five the kernel moves per pixel -- tools/micro/strip_stream.hip: the same
// loads and stores take 2.9 ms per 1024 frames with rows stored whole and 2.2 ms with sector-aligned strips.)  Neighbouring panels
// overlap by 16 columns, so any run of up to 9 consecutive columns lies inside one panel: a reader takes the panel of the run's
// first column.  Row pitch = panels x 256 bytes; the bytes of columns outside the image are never read.
constexpr int GRAY_PANEL_COLS = 240, GRAY_PANEL_BYTES = 256, GRAY_PANEL_LEAD = 8;
OCVAR_HD int gray_pitch(int W) { return ((W + GRAY_PANEL_COLS - 1) / GRAY_PANEL_COLS) * GRAY_PANEL_BYTES; }
OCVAR_HD long long gray_plane_bytes(int W, int H) { return (long long)gray_pitch(W) * H; }
// byte offset of column x (>= 0) in its row, in the panel x belongs to (consecutive columns up to x + 8 follow contiguously)
OCVAR_HD unsigned gray_col(int x) {
    const unsigned p = (unsigned)x / (unsigned)GRAY_PANEL_COLS;
    return p * (unsigned)(GRAY_PANEL_BYTES - GRAY_PANEL_COLS) + (unsigned)x + (unsigned)GRAY_PANEL_LEAD;
}

// What the frame binarise kernel can address of a caller's frame.  binarise.hip::march_unit reads source rows through ONE buffer
// resource of MARCH_SRC_BYTES bytes laid over the frame's first byte: a row's byte offset rv * row_stride travels as a 32-bit
// signed product in the scalar offset, the lane's column offset (at most bpp * (sw - 4), plus the 4 bpp bytes of its load) in the
// vector offset.  The furthest byte a lane reads is byte bpp * sw - 1 of row sh - 1 (sw, sh: width and height rounded down to
// even; the odd last row and column, and the in-place grey, go through 64-bit pointers), so a frame is addressable when
//     (sh - 1) * row_stride + bpp * sw <= MARCH_SRC_BYTES
// -- then the product does not overflow an int, and every load ends inside the resource whether or not the hardware counts the
// scalar offset in its range check.  Beyond it rows would be read at wrapped offsets, or dropped as zeros: a silently different
// detection.  api.hip refuses such frames (OCVAR_E_ARG) before any device call.
constexpr long long MARCH_SRC_BYTES = 0x7fffffffLL;
OCVAR_HD bool frame_src_addressable(int width, int height, long long row_stride, int bpp) {
    const long long sw = width & ~1, sh = height & ~1;
    return sh < 1 || (sh - 1) * row_stride + bpp * sw <= MARCH_SRC_BYTES;
}

// One region of interest handed to the square finder: a whole frame (frame pass) or the clipped
// bounding box of a frame-pass quad (crop pass, opencvar.cpp:682-693).
struct Roi {
    int frame;        // frame index in the batch
    int x0, y0;       // origin inside the frame's gray plane
    int w, h;         // ROI size (img->width/height for the border rule, opencvar.cpp:204-206)
    int sw, sh;       // w & ~1, h & ~1 (opencvar.cpp:158): size of the binary / neighbour plane
    int ns;           // columns of the neighbour plane (sw rounded up to a multiple of 16)
    int owner;        // frame pass: frame index; crop pass: index of the frame-pass quad it came from
    long long nbr_off;  // byte offset of this ROI's neighbour plane (a bit plane on the device) in the pass's pool
};

// A candidate border start found by the binarise kernel.
struct StartCand {
    int roi;
    int pos;          // scan position y*ns + x (ns = plane row stride) at which cvFindContours would discover the border
    int is_hole;
};

// A quad that passed the cvarFindSquares filter.
struct QuadRec {
    int roi;
    int start;        // discovery scan position (orders the sequence: later discovery = earlier in list)
    int pt[8];
};

}  // namespace ocvar
