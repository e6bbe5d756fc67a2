// lane_run.h -- a lane's run of consecutive bytes of one row, held in registers: what the frame kernels (overlay, annotate, patch,
// undistort, yuv, resize, orient, warp, levels, flow) load, unpack, pack and store; the only place that does.  Byte j of a run
// lives in bits 8 (j & 3) of dword j >> 2 (constant indices once unrolled).
#pragma once
#include "hd.h"

namespace ocvar {

OCVAR_D int run_byte(const unsigned* q, int j) { return (int)((q[j >> 2] >> (8 * (j & 3))) & 255u); }
template <int ND>
OCVAR_D void run_put(unsigned (&q)[ND], int j, int b) { q[j >> 2] |= (unsigned)b << (8 * (j & 3)); }

// The lane's run of bytes at p: whole dwords (p is a multiple of 4 then, and all ND dwords belong to the lane), or the first
// nbytes of them byte by byte, the others read as 0 / not written.
template <int ND>
OCVAR_D void run_load(unsigned (&q)[ND], const uint8_t* p, bool dwords, int nbytes) {
    if (dwords) {
        const unsigned* w = reinterpret_cast<const unsigned*>(p);
        OCVAR_UNROLL
        for (int j = 0; j < ND; j++) q[j] = w[j];
    } else {
        OCVAR_UNROLL
        for (int j = 0; j < ND; j++) q[j] = 0;
        OCVAR_UNROLL
        for (int b = 0; b < 4 * ND; b++)
            if (b < nbytes) q[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
    }
}
template <int ND>
OCVAR_D void run_store(const unsigned (&q)[ND], uint8_t* p, bool dwords, int nbytes) {
    if (dwords) {
        unsigned* w = reinterpret_cast<unsigned*>(p);
        OCVAR_UNROLL
        for (int j = 0; j < ND; j++) w[j] = q[j];
    } else {
        OCVAR_UNROLL
        for (int b = 0; b < 4 * ND; b++)
            if (b < nbytes) p[b] = (uint8_t)(q[b >> 2] >> (8 * (b & 3)));
    }
}

// The same for a run of 16-bit little-endian words at an even address (yuv_ex.hip's P010 samples): halfword j lives in bits
// 16 (j & 1) of dword j >> 1, and the traffic that is not by whole dwords is by halfword, the first nhalves of them.
OCVAR_D int run_half(const unsigned* q, int j) { return (int)((q[j >> 1] >> (16 * (j & 1))) & 65535u); }
template <int ND>
OCVAR_D void run_put_half(unsigned (&q)[ND], int j, int h) { q[j >> 1] |= (unsigned)h << (16 * (j & 1)); }
template <int ND>
OCVAR_D void run_load_halves(unsigned (&q)[ND], const uint8_t* p, bool dwords, int nhalves) {
    if (dwords) {
        const unsigned* w = reinterpret_cast<const unsigned*>(p);
        OCVAR_UNROLL
        for (int j = 0; j < ND; j++) q[j] = w[j];
    } else {
        const uint16_t* s = reinterpret_cast<const uint16_t*>(p);
        OCVAR_UNROLL
        for (int j = 0; j < ND; j++) q[j] = 0;
        OCVAR_UNROLL
        for (int h = 0; h < 2 * ND; h++)
            if (h < nhalves) q[h >> 1] |= (unsigned)s[h] << (16 * (h & 1));
    }
}
template <int ND>
OCVAR_D void run_store_halves(const unsigned (&q)[ND], uint8_t* p, bool dwords, int nhalves) {
    if (dwords) {
        unsigned* w = reinterpret_cast<unsigned*>(p);
        OCVAR_UNROLL
        for (int j = 0; j < ND; j++) w[j] = q[j];
    } else {
        uint16_t* s = reinterpret_cast<uint16_t*>(p);
        OCVAR_UNROLL
        for (int h = 0; h < 2 * ND; h++)
            if (h < nhalves) s[h] = (uint16_t)(q[h >> 1] >> (16 * (h & 1)));
    }
}

}  // namespace ocvar
