// grey_pack_emul.cpp -- host build of hd.h's 16-bit grey sum for tests/test_grey_pack_cpu.py.  TEST ONLY.
// gp_sweep walks every (B, G, R) triple through grey_sum16 / grey_low16 with the coefficient words of one byte order and compares
// byte 1 of the sum with BGR2GRAY spelt out, (1868 B + 9617 G + 4899 R + 8192) >> 14; it also reports the largest sum and the
// largest low part, which must both fit 16 bits for the frame kernel's packing (two sums per register, the grey values then
// bytes 1 and 3; tests/test_gpu_grey_pack.py reads the packed plane back).
#include <cstdint>
#include "hd.h"

using namespace ocvar;

extern "C" {

// rev = 0: pixel bytes B G R x with the BGR words; rev = 1: R G B x with the RGB words.  Byte 3 of the pixel (a four-channel
// frame's alpha, weight 0) changes from pixel to pixel.  Returns the number of differing pixels; max_t / max_l: the largest
// grey_sum16 / grey_low16 seen.
long long gp_sweep(int rev, unsigned* max_t, unsigned* max_l) {
    const unsigned KH = rev ? GREY_KH_RGB : GREY_KH_BGR, KL = rev ? GREY_KL_RGB : GREY_KL_BGR;
    long long bad = 0;
    unsigned mt = 0, ml = 0;
    for (unsigned b = 0; b < 256; b++)
        for (unsigned g = 0; g < 256; g++)
            for (unsigned r = 0; r < 256; r++) {
                const unsigned alpha = (b * 7u + g * 13u + r * 29u) & 255u;
                const unsigned px = (rev ? r : b) | (g << 8) | ((rev ? b : r) << 16) | (alpha << 24);
                const unsigned t = grey_sum16(px, KH, KL), l = grey_low16(px, KL);
                const unsigned want = (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14;
                bad += (t >> 8) != want;
                mt = t > mt ? t : mt;
                ml = l > ml ? l : ml;
            }
    *max_t = mt;
    *max_l = ml;
    return bad;
}

}  // extern "C"
