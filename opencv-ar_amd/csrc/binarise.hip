// binarise.hip -- fused grey + pyramid denoise + adaptive threshold + neighbour-mask kernel (gfx950).
//
// Replaces the image stages of cvarFindSquares (/root/reference/src/opencvar.cpp:156-184): cvCloneImage,
// cvPyrDown(5x5), cvPyrUp, cvCvtColor(BGR2GRAY), cvAdaptiveThreshold(GAUSSIAN_C, 7x7, delta 8) -- in frame mode
// also the BGR2GRAY of cvarArMultRegistration (opencvar.cpp:624-627) -- and the local part of cvFindContours
// (opencvar.cpp:183-184): zeroing the 1-px frame and spotting where a border can begin.  The binary image goes out as a bit
// plane in 16x14-pixel tiles with a one-pixel apron (hd.h::nbr_win_off), from which the followers read 8-neighbour masks.
//
// "Wave march": one 64-lane wavefront (a workgroup of its own) owns a strip of 256 columns (4 pixels per lane: 240 output
// columns + an 8-column halo on each side) and walks down a chunk of rows.  Everything vertical lives in registers and nothing
// is a window that is shifted: the vertical pyrDown is two accumulators, the vertical pyrUp two running sums (times four, so a
// finished pixel is the high byte of its sum), the last 8 pyrUp rows a ring of bytes in two registers per pixel that swap names
// every four rows; everything horizontal is a 4-pixel packed word handed to the neighbour lane with a DPP wave shift.  One (unaligned) buffer load per lane and row, reflected columns
// included, two rows under way beyond the current one; rows are addressed through buffer resources (scalar row offset,
// loop-invariant lane offset, stores masked by range).  The image itself never goes through LDS, which only holds a ring of 32
// threshold rows per wave (a nibble per lane) on their way to whole 16x14 bit tiles -- where the border starts of the tile row are
// found on the way, 32 columns at a time (starts_core.h) -- and the staged border starts.  The grey plane is stored in 256-byte panels, one per strip (hd.h::gray_col):
// every store of the kernel is whole 64-byte sectors.  The row body exists in several instances (steady rows in groups of four
// with the ring's position known, strips away from the image edges) so that the hot loop carries no range tests; the filters'
// border rules at the image edges are per-lane byte selectors.
// HBM traffic per pixel: 3 B read (4 B from a four-channel source, 1 B from a grey one) + 1 B grey + 2/7 B of bit plane (frame mode).
// The arithmetic is the integer arithmetic of the definition, so the output is bit-identical:
//   pyrDown  [1 4 6 4 1]^2, (v+128)>>8, BORDER_REFLECT_101        pyrUp  [1 6 1]/[4 4], (v+32)>>6, borders -1->1, n->n-1
//   Gaussian [8 28 56 72 56 28 8]^2, (v+32768)>>16, BORDER_REPLICATE    threshold  src - mean > -8
#include "kernels.h"
#include "starts_core.h"
#include <cstdlib>
#include <type_traits>

#ifndef OCVAR_WAVES_F
#define OCVAR_WAVES_F 5   // waves per SIMD the frame kernel is compiled for (register budget 512 / n, in eights)
#endif
#ifndef OCVAR_ROWS_AHEAD_F
#define OCVAR_ROWS_AHEAD_F 2   // source rows a wave of the frame kernel has under way beyond the one it works on (1 .. 3)
#endif
#ifndef OCVAR_ROWS_AHEAD_F4
#define OCVAR_ROWS_AHEAD_F4 1   // ... with a four-channel source: 16 bytes per lane and row; with two rows ahead its steady loop spills
#endif
#ifndef OCVAR_BIN_WG_WAVES
#define OCVAR_BIN_WG_WAVES 1   // waves per workgroup of the two binarise kernels (1: a wave can take any SIMD with room for it)
#endif
#ifndef OCVAR_ROWS_AHEAD_C
#define OCVAR_ROWS_AHEAD_C 1   // ... of the crop kernel
#endif
#ifndef OCVAR_WAVES_C
#define OCVAR_WAVES_C 5   // ... and the crop kernel
#endif

namespace ocvar {

constexpr int SV = MARCH_STRIP;  // output columns per strip
// Halo: an output pixel's mask depends on source pixels up to 9 columns to its left and 10 to its right (mask 1 (+1 for
// the start test), 7-tap Gaussian 3, pyrUp 3, pyrDown 2), but the stages exchange whole lanes: following the chain lane
// by lane, the first output lane needs the grey of 2 lanes to its left and the last one of 2 lanes to its right -- a third
// lane on the right would only serve the start filter's "row above at x+2" bit of the strip's last column, which is
// dropped instead (the filter is a necessary condition: without it that column merely yields a few more plausible starts).
// 240 output columns: 8 strips across 1920, 16 across 3840.
constexpr int HL = MARCH_HALO_L;   // (MARCH_HALO_R lanes on the right: static_assert in kernels.h ties both to the strip)
constexpr int RING_ROWS = 32;   // threshold rows a wave keeps in LDS (march_unit::flush_due): a tile row's 16 and the rows of one more group

// A value that is the same in all lanes of the wave, moved to an SGPR.  The work-unit index comes from threadIdx.x >> 6,
// which the compiler must treat as per-lane: without this every row counter of the march lives in a VGPR, every loop
// test is a VALU compare + EXEC mask, and every row address is 64-bit VALU arithmetic.
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// a wave-uniform 64-bit offset, pinned to an SGPR pair (row offsets: the per-lane part of an address is then a 32-bit add)
__device__ __forceinline__ long long wave_uniform64(long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// buffer resource over [p, p + bytes): raw (stride 0), 32-bit data format -- the addressing mode of the row loads and stores
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
constexpr int BUF_NT = 2;   // cache policy "non-temporal" of the buffer builtins

__device__ __forceinline__ int reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

__device__ __forceinline__ unsigned grey_of(unsigned b, unsigned g, unsigned r) { return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14; }

// lane i receives lane i-1 / lane i+1 (DPP whole-wave shifts: one VALU move, no LDS traffic)
__device__ __forceinline__ unsigned up1(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true); }
__device__ __forceinline__ unsigned down1(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true); }

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ us2 as_us2(unsigned v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ unsigned as_u32(us2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_udot4(a, b, c, false); }
__device__ __forceinline__ unsigned dot2(us2 a, unsigned k, unsigned c) { return __builtin_amdgcn_udot2(a, as_us2(k), c, false); }
constexpr unsigned K2(unsigned lo, unsigned hi) { return lo | (hi << 16); }
__device__ __forceinline__ unsigned alignb(unsigned hi, unsigned lo, unsigned sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
__device__ __forceinline__ unsigned byte_of(unsigned v, int j) { return (v >> (8 * j)) & 255u; }
__device__ __forceinline__ unsigned long long rotl64(unsigned long long v, unsigned s) { return s ? (v << s) | (v >> (64u - s)) : v; }
// nib = 2 * nib + (floor(S / 65536) < byte B of w): the threshold test of one pixel, the operands picked by the instruction itself
// (SDWA: the high word of S sign-extended, one byte of w) -- one compare and one add-with-carry, no operand to prepare.
template <int B>
__device__ __forceinline__ void push_bit(unsigned& nib, unsigned S, unsigned w) {
    static_assert(B >= 0 && B < 4, "byte of a dword");
    if constexpr (B == 0) asm("v_cmp_lt_i32_sdwa vcc, sext(%1), %2 src0_sel:WORD_1 src1_sel:BYTE_0\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(nib) : "v"(S), "v"(w) : "vcc");
    if constexpr (B == 1) asm("v_cmp_lt_i32_sdwa vcc, sext(%1), %2 src0_sel:WORD_1 src1_sel:BYTE_1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(nib) : "v"(S), "v"(w) : "vcc");
    if constexpr (B == 2) asm("v_cmp_lt_i32_sdwa vcc, sext(%1), %2 src0_sel:WORD_1 src1_sel:BYTE_2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(nib) : "v"(S), "v"(w) : "vcc");
    if constexpr (B == 3) asm("v_cmp_lt_i32_sdwa vcc, sext(%1), %2 src0_sel:WORD_1 src1_sel:BYTE_3\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(nib) : "v"(S), "v"(w) : "vcc");
}

// nib = (floor(S / 65536) < byte B of w): the first pixel's test starts the nibble (no register to clear)
template <int B>
__device__ __forceinline__ void first_bit(unsigned& nib, unsigned S, unsigned w) {
    static_assert(B >= 0 && B < 4, "byte of a dword");
    if constexpr (B == 0) asm("v_cmp_lt_i32_sdwa vcc, sext(%1), %2 src0_sel:WORD_1 src1_sel:BYTE_0\n\tv_cndmask_b32_e64 %0, 0, 1, vcc" : "=v"(nib) : "v"(S), "v"(w) : "vcc");
    if constexpr (B == 1) asm("v_cmp_lt_i32_sdwa vcc, sext(%1), %2 src0_sel:WORD_1 src1_sel:BYTE_1\n\tv_cndmask_b32_e64 %0, 0, 1, vcc" : "=v"(nib) : "v"(S), "v"(w) : "vcc");
    if constexpr (B == 2) asm("v_cmp_lt_i32_sdwa vcc, sext(%1), %2 src0_sel:WORD_1 src1_sel:BYTE_2\n\tv_cndmask_b32_e64 %0, 0, 1, vcc" : "=v"(nib) : "v"(S), "v"(w) : "vcc");
    if constexpr (B == 3) asm("v_cmp_lt_i32_sdwa vcc, sext(%1), %2 src0_sel:WORD_1 src1_sel:BYTE_3\n\tv_cndmask_b32_e64 %0, 0, 1, vcc" : "=v"(nib) : "v"(S), "v"(w) : "vcc");
}

struct MarchOut {
    uint8_t* gray;          // frame mode: grey plane of this frame (stride gray_stride), else null
    long long gray_stride;
    uint8_t* nbr;           // bit plane of this ROI (hd.h::nbr_win_off), ns columns
    int ns;
    int roi;
    StartCand* cands;
    int* n_cands;
    int cap_cands;
    int* err;
};

// Sources of march_unit: the caller's frame in one of the formats of include/ocvar_hip.h (OCVAR_FMT_*: frame mode, which
// also writes the grey plane), or SRC_CROP, a crop of the frame's panelled grey plane (hd.h::gray_col).
constexpr int SRC_CROP = 5;
// (the kernels' own constant form of frames_core.h::format_bpp, and 1 for SRC_CROP, which is no format)
constexpr int src_bpp(int src) { return src == OCVAR_FMT_BGR || src == OCVAR_FMT_RGB ? 3 : src == OCVAR_FMT_BGRA || src == OCVAR_FMT_RGBA ? 4 : 1; }
static_assert(src_bpp(0) == format_bpp(0) && src_bpp(1) == format_bpp(1) && src_bpp(2) == format_bpp(2) && src_bpp(3) == format_bpp(3) && src_bpp(4) == format_bpp(4), "one table");

// One work unit: strip `strip` of an (sw x sh) ROI, output rows [Y0, Y1).
// SRC: what `src` holds (above).  BGR / RGB: one 12-byte load per lane and row; BGRA / RGBA: one 16-byte load (four whole
// pixels); GRAY and crops: one 4-byte load.
// EDGE = false: the strip lies strictly inside the image (no lane holds a column < 0 or >= sw), so the border rules of the
// filters and their lane masks are compiled out -- six of a 1080p frame's eight strips; a crop's strips always touch an edge.
template <int SRC, bool EDGE>
__device__ void march_unit(const uint8_t* src, long long src_stride, int x_org /* crops: the ROI's first column in the frame's grey plane */, int sw, int sh, int strip, int Y0, int Y1, const MarchOut& o,
                           unsigned* stage, uint8_t* rowbuf /* LDS, RING_ROWS rows x 64 lanes */) {
    constexpr bool FRAME = SRC != SRC_CROP;
    constexpr int BPP = src_bpp(SRC);   // bytes per source pixel
    constexpr bool FOUR = BPP == 4;
    const int lane = threadIdx.x & 63;
    const int XS = strip * SV - 4 * HL;
    const int c0 = XS + 4 * lane;
    const int pw = sw >> 1, ph_ = sh >> 1;
    const int k0 = c0 >> 1;  // pyramid column of the lane's first pyramid sample (c0 is a multiple of 4)
    const bool needed = !EDGE || (c0 + 3 >= -16 && c0 < sw + 16);  // beyond every halo: never consumed
    const bool fast = !EDGE || (c0 >= 0 && c0 + 3 < sw);
    const bool aligned = FRAME ? ((src_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) : true;
    // (wave-uniform flags as scalars: left as they are the compiler keeps them as lane masks and re-derives their negations with
    // vector instructions in every row)
    // The filters' border rules at the image's left and right edge are byte selections in the one or two lanes that hold the edge
    // columns; every lane carries its selectors (the identity elsewhere), so the row body needs no wave-uniform "this strip touches
    // an edge" tests -- as flags those cost scalar registers the kernel does not have, and a handful of vector instructions per row
    // to re-derive their negations.  (v_perm_b32: bytes 0..3 = the second operand, 4..7 = the first.)
    constexpr unsigned SEL_ID = 0x03020100u;
    // pyrUp's right border, "pyramid column pw stands for column pw-1", on the lane's pair (P[k0], P[k0+1]) with the left lane's pair as first operand
    const unsigned selP = !EDGE ? SEL_ID : k0 + 1 == pw ? 0x01000100u : k0 == pw ? 0x03020706u : SEL_ID;
    // BORDER_REPLICATE of the 7x7 Gaussian, applied to the vertical sums (a replicated column's sums are the edge column's): the lane
    // that holds column 0 takes (V0, V0) for what it would receive from its left neighbour; the lane that holds column sw-1 (its
    // pixel 1 or 3: sw is even) first overwrites its own pair (V2, V3) when those lie beyond the edge, then takes its last real
    // column for what it would receive from the right.
    const unsigned selL = EDGE && c0 == 0 ? 0x05040504u : SEL_ID;
    const unsigned selB = EDGE && c0 + 2 == sw ? 0x07060706u : SEL_ID;
    const unsigned selR = EDGE && c0 < sw && c0 + 4 >= sw ? 0x07060706u : SEL_ID;
    // byte offset of source column c (0 <= c < sw) in its row: BPP c in a frame (3 c BGR); in the panelled grey plane (hd.h::gray_col)
    // the crop's column c is the frame's column x_org + c (up to 9 consecutive columns follow contiguously from any column)
    auto col_off = [&](int c) -> unsigned { return FRAME ? (unsigned)(BPP * c) : gray_col(x_org + c); };
    // reflected source columns of the lanes that straddle an image edge (BORDER_REFLECT_101)
    unsigned xr0 = 0, xr1 = 0, xr2 = 0, xr3 = 0;
    if (needed && !fast) {
        xr0 = col_off(reflect101(c0, sw));
        xr1 = col_off(reflect101(c0 + 1, sw));
        xr2 = col_off(reflect101(c0 + 2, sw));
        xr3 = col_off(reflect101(c0 + 3, sw));
    }
    // Load plan: every lane loads its 4 pixels with ONE (unaligned) load per row -- 4 bytes grey, 12 bytes BGR, 16 BGRA -- also the
    // lanes that hold reflected columns, whose 4 (grey) bytes are then permuted.  With BORDER_REFLECT_101 a lane left of
    // column 0 holds columns -c0 .. -c0-3, a lane right of column sw-1 holds 2sw-2-c0 .. 2sw-5-c0: four contiguous source
    // pixels in reverse order; the lane that straddles the right edge (sw - c0 == 2: sw is even, c0 a multiple of 4) holds
    // c0, c0+1, c0, c0-1 and loads c0-2 .. c0+1.  (The byte loads of the generic path sit in a divergent branch, which makes
    // every row wait for its own loads instead of running a row ahead: a crop has edge lanes on both sides of every work
    // unit, and its binarise kernel was latency-bound by that.)  No byte outside columns 0 .. sw-1 of the row is read.
    const bool plan = sw >= 32;   // single reflection, every offset inside the row
    unsigned goff = col_off(0), gsel = 0x03020100u;
    if (plan && needed) {   // (first column of the lane's load)
        if (c0 + 3 < 0) { goff = col_off(-c0 - 3); gsel = 0x00010203u; }
        else if (c0 >= sw) { goff = col_off(2 * sw - 5 - c0); gsel = 0x00010203u; }
        else if (c0 + 3 >= sw) { goff = col_off(c0 - 2); gsel = 0x01020302u; }
        else goff = col_off(c0);
    }
    // per-lane byte offsets (unsigned: the row bases are wave-uniform, so loads/stores can use the SGPR-base + 32-bit VGPR offset form)
    const unsigned src_off = fast ? col_off(c0) : col_off(0);
    // Rows are addressed through buffer resources: base in four SGPRs, the row's byte offset in one SGPR (one s_mul per row), the
    // lane's offset in a loop-invariant VGPR -- no 64-bit address arithmetic, no per-lane pointers to keep or spill.  A lane that
    // must not store gets an offset beyond the resource's size: the hardware drops its store, so the grey and mask stores need
    // no EXEC mask and the row body stays one basic block.
    constexpr unsigned OOB = 0x80000000u;   // >= every resource size below (+ 16 does not wrap)
    const __amdgpu_buffer_rsrc_t src_rs = make_rsrc(src, (unsigned)MARCH_SRC_BYTES);   // (hd.h::frame_src_addressable: what api.hip lets through)
    const __amdgpu_buffer_rsrc_t gray_rs = make_rsrc(o.gray, o.gray ? (unsigned)(o.gray_stride * sh) : 0u);
    const __amdgpu_buffer_rsrc_t nbr_rs = make_rsrc(o.nbr, (unsigned)nbr_plane_bytes(o.ns, sh));
    // the grey plane's panel of this strip (hd.h::gray_col): all 64 lanes store, 256 contiguous bytes at a 256-byte boundary -- the
    // halo lanes' bytes are the neighbouring strips' columns again (same values), or columns outside the image (never read)
    const unsigned out_off = (unsigned)(strip * GRAY_PANEL_BYTES + 4 * lane);
    unsigned colmask = 0;  // which of the lane's 4 columns lie inside cvFindContours' zeroed frame
    for (int j = 0; j < 4; j++) colmask |= (!EDGE || (c0 + j >= 1 && c0 + j <= sw - 2)) ? (1u << j) : 0u;
    // Border starts are staged per wave in LDS and appended to the global list with ONE atomic per flush: a
    // single list counter only sustains ~90 atomics/us chip-wide, which one atomic per image row would exceed.
    int staged = 0;  // wave-uniform
    auto flush = [&]() {
        if (staged == 0) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        int base = 0;
        if (lane == 0) base = atomicAdd(o.n_cands, staged);
        base = wave_uniform(base);
        for (int i = lane; i < staged; i += 64) {
            const unsigned e = stage[i];
            if (base + i < o.cap_cands) {
                StartCand sc;
                sc.roi = o.roi;
                sc.pos = (int)(e & 0x7fffffffu);
                sc.is_hole = (int)(e >> 31);
                o.cands[base + i] = sc;
            } else {
                atomicOr(o.err, ERR_CAND_OVERFLOW);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        staged = 0;
    };

    // The bit plane (hd.h::nbr_win_off) is written a tile row at a time: threshold rows go to a ring of RING_ROWS rows in LDS (one
    // byte per lane and row: its nibble), and when row 14 ty + 14 is in, the 16 rows 14 ty - 1 .. 14 ty + 14 of tile row ty are made
    // into the strip's 15 tiles -- 960 contiguous bytes, ONE store instruction: lane l (< 60) stores dwords 4 (l & 3) .. 4 (l & 3) + 3
    // of tile l >> 2, so every 64-byte sector is written whole by four neighbouring lanes.  (A row at a time would be pieces of
    // 15 sectors per wave, and on this hardware a store issued in every iteration makes the loop-top wait for the prefetched
    // source row wait for that store too: vmcnt counts loads and stores in order.)  A tile's dword is 18 columns, 16 tx - 1 ..
    // 16 tx + 16: the nibbles of lanes 4 tx + 1 .. 4 tx + 6 -- the apron columns -1 and 240 of a strip are the threshold bits of
    // halo lanes 1 and 62, which the wave computes anyway; rows Y0 - 1 and Y1, the apron rows of a unit, are computed for the
    // start tests.  Y0 is a multiple of 14 (plan_core.h / MARCH_CROP_ROWS), so a tile row belongs to one work unit; rows outside
    // [0, Y1] (row -1, rows below the image) are stored as 0.
    // The same words, 32 columns of a row each, are where the tile row's border starts are found (starts_core.h): every lane tests
    // the rows it assembles anyway against the row above -- its own previous word, or the last word of the lane before it in the
    // quad -- which is ~8 vector instructions per image row of the wave, against a window, a table read and a ballot per row and
    // lane; and the starts are then staged one per lane and turn, so the cost follows the starts that exist.
    const int tile_s = strip * (SV / NBR_TILE_W) + (lane >> 2);   // the lane's tile in the tile row
    const unsigned flush_src = (unsigned)(lane < 60 ? lane >> 2 : 14) * 4u;   // byte of lane 4 tx in an LDS row (lanes 60..63: any tile, their store is dropped)
    const unsigned flush_dst = lane < 60 && tile_s * NBR_TILE_W < o.ns ? (unsigned)tile_s * NBR_TILE_BYTES + (unsigned)(lane & 3) * 16u : OOB;
    auto flush_tiles = [&](int ty) {   // the rows of tile row ty are in the ring
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        // (what only this block needs of the lane's place is worked out here, from a copy of the lane id the compiler cannot see
        // through: kept in registers across the row loop instead, it would cost the loop registers it does not have)
        int fl = lane;
        asm volatile("" : "+v"(fl));
        const int ftx = fl >> 2, fq = fl & 3;
        const unsigned wbits = starts_word_bits(ftx);
        unsigned w[4];
        {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));   // (non-temporal stores: written once, read much later)
            v4u d;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r = NBR_TILE_H * ty + 4 * (lane & 3) + i - 1;   // image row of dword 4 (l & 3) + i
                const unsigned* p = reinterpret_cast<const unsigned*>(rowbuf + (r & (RING_ROWS - 1)) * 64 + flush_src);   // nibbles of lanes 4 tx .. 4 tx + 7, a byte each
                const unsigned p0 = p[0], p1 = p[1];
                // two nibbles per byte (bytes 0 and 2 of each word), those four bytes into one word: columns 16 tx - 8 .. 16 tx + 23
                const unsigned ww = __builtin_amdgcn_perm(p1 | (p1 >> 4), p0 | (p0 >> 4), 0x06040200u);
                w[i] = (unsigned)r <= (unsigned)Y1 ? ww & wbits : 0u;   // (rows the unit did not write: stale ring rows)
                d[i] = (w[i] >> 7) & 0x3ffffu;
            }
            const unsigned so = (unsigned)wave_uniform((int)nbr_tile_off(0u, (unsigned)ty, o.ns));
            // The tile row's offset is added to the lanes' offsets, the scalar offset field stays 0.  A store of more than 64 bits
            // must not be followed at once by a vector instruction that writes its data registers; the compiler's hazard
            // recogniser inserts the wait state only for buffer stores WITHOUT a register in the scalar offset field (with one the
            // ISA manual promises no hazard) -- and gfx950 has it all the same: with the offset in an SGPR a register copy the
            // allocator placed right behind the store overwrote its first data dword now and then (only while the memory system
            // was busy: frames >= 16 of a batch).  (OOB + so < 2^32: dropped all the same.)
            __builtin_amdgcn_raw_buffer_store_b128(d, nbr_rs, (int)(flush_dst + so), 0, BUF_NT);
        }
        // Plausible border starts of the tile row's rows [14 ty, min(14 ty + 14, Y1)) (sparse), staged as y * ns + x with the hole
        // flag in bit 31: each turn of the loop takes one start from every lane that still has one.
        const int nrows = wave_uniform(Y1 - NBR_TILE_H * ty < NBR_TILE_H ? Y1 - NBR_TILE_H * ty : NBR_TILE_H);
        const int col0 = strip * SV + NBR_TILE_W * ftx;
        const unsigned own = fl < 60 ? (EDGE ? starts_own_bits(col0, sw) : STARTS_OWN_BITS) : 0u;
        unsigned long long any, hole;
        starts_of_lane(w, up1(w[3]), 4 * fq - 1, nrows, own, any, hole);
        const unsigned pos0 = (unsigned)((NBR_TILE_H * ty + 4 * fq - 1) * o.ns + col0);   // (the apron row of tile row 0 is row -1: never a start row)
#pragma nounroll
        for (;;) {
            const unsigned long long mask = __ballot(any != 0ull);
            const int n = wave_uniform(__popcll(mask));
            if (n == 0) break;
            if (staged + n > MARCH_STAGE) flush();
            if (any != 0ull) {
                const unsigned k = (unsigned)__builtin_ctzll(any);
                stage[staged + __popcll(mask & ((1ull << lane) - 1ull))] = (pos0 + (k >> 4) * (unsigned)o.ns + (k & 15u)) | ((unsigned)(hole >> k) << 31);
                any &= any - 1ull;
            }
            staged += n;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    };
    // Tile rows are flushed between rows: the ring holds RING_ROWS = 32 rows, so a tile row's 16 rows are still there when up to
    // four more have come in, and the flush -- with the start test some 200 instructions -- stands once behind each group of rows
    // instead of behind every row of it (a 16-row ring needs the flush at the very row that completes the tile row: eight copies
    // in the steady loop, and code size is speed here).  y_in: the last threshold row written to the ring.
    int y_in = Y0 - 2, ty_next = Y0 / NBR_TILE_H;
    const int ty_end = (Y1 + NBR_TILE_H - 1) / NBR_TILE_H;
    auto flush_due = [&]() {   // a tile row is complete with its row 14 ty + 14, the unit's last one with row Y1
#pragma nounroll
        while (ty_next < ty_end && y_in >= (NBR_TILE_H * ty_next + NBR_TILE_H < Y1 ? NBR_TILE_H * ty_next + NBR_TILE_H : Y1)) {
            flush_tiles(ty_next);
            ty_next++;
        }
    };

    // raw source words of virtual row v (3 dwords BGR / 4 dwords BGRA / 1 dword grey for fast lanes, 4 pixels for edge lanes)
    struct Raw3 { unsigned d0, d1, d2; };
    struct Raw4 { unsigned d0, d1, d2, d3; };
    using Raw = typename std::conditional<FOUR, Raw4, Raw3>::type;
    auto fetch = [&](int v, bool inside /* 0 <= v < sh is known; only asked for when the load plan holds (steady rows) */) -> Raw {
        Raw r = {0u, 0u, 0u};
        const int rv = inside ? v : reflect101(v, sh);
        if (inside || plan) {
            const int so = wave_uniform(rv * (int)src_stride);   // (< 2^31: a frame, or rows of the grey plane from the crop's origin on)
            if constexpr (BPP == 3) {   // one (unaligned) buffer_load_dwordx3.  Not non-temporal: with the hint the kernel is 7 % slower alone on the GPU
                         // (5.8 against 5.4 ms per 2048 frames: the halo columns two strips share stop hitting in the L2); the grey
                         // and mask STORES carry it (+2 % with four contexts, round 3)
                typedef unsigned v3u __attribute__((ext_vector_type(3)));
                const v3u d = __builtin_amdgcn_raw_buffer_load_b96(src_rs, (int)goff, so, 0);
                r.d0 = d.x; r.d1 = d.y; r.d2 = d.z;
            } else if constexpr (FOUR) {   // one buffer_load_dwordx4: four whole pixels, a dword each
                typedef unsigned v4u __attribute__((ext_vector_type(4)));
                const v4u d = __builtin_amdgcn_raw_buffer_load_b128(src_rs, (int)goff, so, 0);
                r.d0 = d.x; r.d1 = d.y; r.d2 = d.z; r.d3 = d.w;
            } else {     // grey frames, and crops: ordinary loads -- the two concentric quads of a marker give two crops over nearly the same pixels
                r.d0 = __builtin_amdgcn_raw_buffer_load_b32(src_rs, (int)goff, so, 0);
            }
            return r;
        }
        const uint8_t* row = src + wave_uniform64((long long)rv * src_stride);
        if (!needed) return r;
        auto bytes4 = [](const uint8_t* p) -> unsigned { return p[0] | (p[1] << 8) | (p[2] << 16) | ((unsigned)p[3] << 24); };
        if (fast) {
            if constexpr (BPP == 3) {
                if (aligned) {
                    const unsigned* p = reinterpret_cast<const unsigned*>(row + src_off);
                    r.d0 = p[0]; r.d1 = p[1]; r.d2 = p[2];
                } else {
                    const uint8_t* p = row + src_off;
                    r.d0 = p[0] | (p[1] << 8) | (p[2] << 16) | ((unsigned)p[3] << 24);
                    r.d1 = p[4] | (p[5] << 8) | (p[6] << 16) | ((unsigned)p[7] << 24);
                    r.d2 = p[8] | (p[9] << 8) | (p[10] << 16) | ((unsigned)p[11] << 24);
                }
            } else if constexpr (FOUR) {
                const uint8_t* p = row + src_off;
                if (aligned) {
                    const unsigned* q = reinterpret_cast<const unsigned*>(p);
                    r.d0 = q[0]; r.d1 = q[1]; r.d2 = q[2]; r.d3 = q[3];
                } else {
                    r.d0 = bytes4(p); r.d1 = bytes4(p + 4); r.d2 = bytes4(p + 8); r.d3 = bytes4(p + 12);
                }
            } else if constexpr (FRAME) {   // a grey frame: nothing beyond the lane's 4 bytes is read (the row may end there)
                const uint8_t* p = row + src_off;
                r.d0 = aligned ? *reinterpret_cast<const unsigned*>(p) : bytes4(p);
            } else {
                const uintptr_t a = reinterpret_cast<uintptr_t>(row + src_off);
                const unsigned* p = reinterpret_cast<const unsigned*>(a & ~(uintptr_t)3);
                r.d0 = alignb(p[1], p[0], (unsigned)(a & 3));
            }
        } else if constexpr (BPP == 3) {  // pack the 4 reflected pixels into the same 12-byte layout
            const uint8_t *p0 = row + xr0, *p1 = row + xr1, *p2 = row + xr2, *p3 = row + xr3;
            r.d0 = p0[0] | (p0[1] << 8) | (p0[2] << 16) | ((unsigned)p1[0] << 24);
            r.d1 = p1[1] | (p1[2] << 8) | (p2[0] << 16) | ((unsigned)p2[1] << 24);
            r.d2 = p2[2] | (p3[0] << 8) | (p3[1] << 16) | ((unsigned)p3[2] << 24);
        } else if constexpr (FOUR) {      // a dword per pixel (the fourth byte is not read: its coefficient is 0)
            const uint8_t *p0 = row + xr0, *p1 = row + xr1, *p2 = row + xr2, *p3 = row + xr3;
            r.d0 = p0[0] | (p0[1] << 8) | (p0[2] << 16);
            r.d1 = p1[0] | (p1[1] << 8) | (p1[2] << 16);
            r.d2 = p2[0] | (p2[1] << 8) | (p2[2] << 16);
            r.d3 = p3[0] | (p3[1] << 8) | (p3[2] << 16);
        } else {
            r.d0 = row[xr0] | (row[xr1] << 8) | (row[xr2] << 16) | ((unsigned)row[xr3] << 24);
        }
        return r;
    };
    auto to_grey = [&](const Raw& r) -> unsigned {
        if constexpr (BPP == 1) return r.d0;   // (grey frames: BGR2GRAY of B = G = R = g is g)
        // (1868 B + 9617 G + 4899 R + 8192) >> 14 with everything times four: (7472 B + 38468 G + 19596 R + 32768) >> 16.  Coefficient
        // halves for v_dot4_u32_u8 (hd.h::GREY_KH_BGR ...): 7472 = 29*256+48, 38468 = 150*256+68, 19596 = 76*256+140; in reverse
        // byte order for RGB sources; 0 on byte 3 (a four-channel pixel's alpha).  The grey value is byte 1 of hd.h::grey_sum16,
        // T = (dot4(KH) + 128) + byte 1 of dot4(KL) < 2^16: three instructions per pixel, the add picking the byte itself -- and the
        // add of every second pixel writes the upper word of the register of the pixel before it, so that the four grey values
        // are bytes 1 and 3 of two registers and ONE byte permute packs them (no shift per pixel, no OR).
        constexpr bool REV = SRC == OCVAR_FMT_RGB || SRC == OCVAR_FMT_RGBA;
        const unsigned KH = REV ? GREY_KH_RGB : GREY_KH_BGR, KL = REV ? GREY_KL_RGB : GREY_KL_BGR;
        // The four pixels' twelve instructions are one block, in an order of its own.  On this hardware a dot product's result may
        // be read by another kind of vector instruction only three instructions later, and a register of which an instruction
        // wrote one half only one wait state later; the compiler keeps both distances in its own code and cannot see into a
        // block -- so all eight products come first, then the four sums in the products' order (the last sum reads the eighth
        // product with three sums between them), then the wait state.  (Left to the compiler with only the sums as blocks, the
        // products of two rows went above the row loop's branch, where sixteen of them stayed live: spills.)  The permute is the
        // compiler's own: it knows what the lane shifts that read the result next have to wait for.
        auto grey4 = [](unsigned w0, unsigned w1, unsigned w2, unsigned w3, unsigned kh, unsigned kl, unsigned kh3, unsigned kl3) -> unsigned {
            unsigned g, t, l0, h1, l1, l2, h3, l3;   // g, t: high sums of pixels 0 and 2, then the sums of pixels 0 | 1 and 2 | 3
            asm("v_dot4_u32_u8 %0, %8, %12, %16\n\t"
                "v_dot4_u32_u8 %2, %8, %13, 0\n\t"
                "v_dot4_u32_u8 %3, %9, %12, %16\n\t"
                "v_dot4_u32_u8 %4, %9, %13, 0\n\t"
                "v_dot4_u32_u8 %1, %10, %12, %16\n\t"
                "v_dot4_u32_u8 %5, %10, %13, 0\n\t"
                "v_dot4_u32_u8 %6, %11, %14, %16\n\t"
                "v_dot4_u32_u8 %7, %11, %15, 0\n\t"
                "v_add_u32_sdwa %0, %0, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"
                "v_add_u32_sdwa %0, %3, %4 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_1\n\t"
                "v_add_u32_sdwa %1, %1, %5 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"
                "v_add_u32_sdwa %1, %6, %7 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_1\n\t"
                "s_nop 0"
                : "=&v"(g), "=&v"(t), "=&v"(l0), "=&v"(h1), "=&v"(l1), "=&v"(l2), "=&v"(h3), "=&v"(l3)
                : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(kh), "s"(kl), "s"(kh3), "s"(kl3), "v"(128u));
            return __builtin_amdgcn_perm(t, g, 0x07050301u);   // bytes 1 and 3 of g, bytes 1 and 3 of t
        };
        if constexpr (FOUR) return grey4(r.d0, r.d1, r.d2, r.d3, KH, KL, KH, KL);   // a dword per pixel: no byte alignment
        // bytes b0 g0 r0 (x) | b1 g1 r1 (x) | b2 g2 r2 (x) | (x) b3 g3 r3
        return grey4(r.d0, alignb(r.d1, r.d0, 3), alignb(r.d2, r.d1, 2), r.d2, KH, KL, KH << 8, KL << 8);
    };

    // Pyramid rows the unit needs: from qa (two rows before the first pyrUp row, Y0 - 4, that its first threshold row reads) to qb.
    // At the image's top the rows above 0 are copies of row 0 (BORDER_REPLICATE), so nothing before pyramid row -1 is read; at its
    // bottom the last pyrUp rows, sh - 2 and sh - 1, come with pyramid row sh / 2 (= row sh / 2 - 1 again) and the rows below are
    // copies: four source rows less at either end than the general formula asks for (a crop of 170 rows: 8 of 187).
    const int qa = Y0 == 0 ? -1 : Y0 / 2 - 3, qb = (Y1 + 3) / 2 + 1 < sh / 2 ? (Y1 + 3) / 2 + 1 : sh / 2;
    const int v_first = 2 * qa - 2, v_last = 2 * qb + 2;
    // Vertical pyrDown [1 4 6 4 1] by accumulation: pyramid row k (centre: source row 2k) is complete with source row 2k+2.  An
    // even row 2k gives 1 to row k-1 (which it completes), 6 to row k, 1 to row k+1; an odd row gives 4 to its two neighbours.
    // accA collects the row that completes next, accB the one after it (with the rounding constant): no 5-row window to shift.
    us2 accA = as_us2(0u), accB = as_us2(0u);   // packed pairs (column c0 | column c0+2 << 16), <= 16 * 4080 + 128
    unsigned prevP = 0;                      // previous pyramid row for the bottom border
    // Vertical pyrUp, all values times four so that a finished pixel is the HIGH byte of its 16-bit sum (no shift; the ring insert
    // picks that byte): with r(q) the horizontally up-sampled pyramid row q times 4 (even columns r0|r2<<16, odd r1|r3<<16),
    // pyrUp row 2(q-1)   = (r(q-2) + 6 r(q-1) + r(q) + 128) >> 8,   pyrUp row 2(q-1)+1 = (4 (r(q-1) + r(q)) + 128) >> 8
    // (the definition's (x + 32) >> 6 with x times 4; <= 4 * 16320 + 128 < 2^16).  Kept between rows: T = r(q-2) + 6 r(q-1) + 128
    // and b = r(q-1) + 128 -- a new row costs one add for the even row, an add and a multiply-add for the odd row, two for the state.
    us2 Te = as_us2(0u), To = as_us2(0u), be = as_us2(0u), bo = as_us2(0u);
    // The last 8 (virtual) pyrUp rows, one pair of registers per pixel with a row per byte, kept as a RING: virtual row vu goes
    // to byte vu & 3 of wa[p], which holds the current group of four rows (and, in the bytes not yet overwritten, the group
    // before the previous one); wb[p] holds the previous group; when a group begins the two words change names (v_swap_b32).
    // A new row is one byte permute per pixel (it overwrites a row that has left the window; nothing is shifted), the vertical
    // 7-tap Gaussian of a pixel is two v_dot4_u32_u8 whose coefficient words are the kernel rotated to the ring's position,
    // and the threshold's source byte (row vu-3) is picked by the compare itself.  In the steady rows the position is a
    // compile-time constant (the loop is unrolled over 4 rows); the rows at the top and bottom of a unit compute selectors
    // and coefficients on the scalar unit.  (An 8-row ring without the renaming needs the loop unrolled over 8 rows: with the
    // two instances of this function in one kernel that was 52 KB of code and 30 % slower -- instruction cache.)
    unsigned wa[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};

    // One source row.  S ("steady"): v lies where every range test below has a known outcome -- the rows it completes are
    // inside the work unit and away from the image's first and last rows -- so the tests (a scalar compare and branch
    // each, dozens per row) are compiled out; the rows at the top and bottom of a unit take the generic instance.
    // Source rows in flight per wave: AHEAD rows beyond the one being worked on (frames: 2, crops: 1).  With one row under way the
    // ~6 K resident waves have 4.7 MB in flight, which at the latency of a loaded memory system caps the frame kernel near 4 TB/s;
    // and when other contexts' kernels hold half of the wave slots the frame kernel's waves must each keep more in flight to
    // keep the memory system busy.
    constexpr int AHEAD = !FRAME ? OCVAR_ROWS_AHEAD_C : FOUR ? OCVAR_ROWS_AHEAD_F4 : OCVAR_ROWS_AHEAD_F;
    Raw nxt = fetch(v_first, false), nxt2 = fetch(v_first + 1, false), nxt3 = {0u, 0u, 0u}, nxt4 = {0u, 0u, 0u};
    if (AHEAD >= 2) nxt3 = fetch(v_first + 2, false);
    if (AHEAD >= 3) nxt4 = fetch(v_first + 3, false);
    auto row = [&](const int v, auto steady_tag, auto parity_tag, auto ring_tag) {
        constexpr bool S = decltype(steady_tag)::value;
        constexpr int PAR = decltype(parity_tag)::value;   // 1: v is odd, 2: v is even, 0: not known at compile time
        constexpr int VM = decltype(ring_tag)::value;      // v & 3 of an even steady row (the ring position follows from it), -1: not known
        // Two rows in flight per wave (with one, the ~6 K resident waves have 4.7 MB under way, which at the latency of a loaded
        // memory system caps the kernel near 4 TB/s): this row's words were loaded two rows ago, and the row after the next is
        // requested as soon as they have been turned into grey -- into the registers they leave, so the two sets swap names
        // every row and nothing is copied (loaded before, a third set was live and the sets rotated through moves).
        unsigned g = to_grey(nxt);
        if (FRAME) asm volatile("" : "+v"(g) : : "memory");   // (keeps the load below this point, and the conversion above it)
        else asm volatile("" : : : "memory");
        // (the request goes into the registers the converted row leaves: the sets swap names, nothing is copied in the unrolled loop)
        if (AHEAD == 1) {
            nxt = nxt2;
            if (S || v + 1 < v_last) nxt2 = fetch(v + 2, S);
        } else if (AHEAD == 2) {
            nxt = nxt2; nxt2 = nxt3;
            if (S || v + 2 < v_last) nxt3 = fetch(v + 3, S);
        } else {
            nxt = nxt2; nxt2 = nxt3; nxt3 = nxt4;
            if (S || v + 3 < v_last) nxt4 = fetch(v + 4, S);
        }
        if (EDGE && (S || plan)) g = __builtin_amdgcn_perm(g, g, gsel);   // (gsel: the identity in lanes that hold no reflected columns)
        // (a 32-bit store reads its data register as it issues: unlike the 128-bit tile stores in flush_tiles it may keep the row's
        // offset in the scalar offset field; test_planes_of_every_frame_of_a_busy_batch compares the grey plane too)
        if (FRAME && (S || (v >= Y0 && v < Y1)))   // (the frame pass, which always has a grey plane) rows [Y0,Y1) are real rows, each loaded exactly once
            __builtin_amdgcn_raw_buffer_store_b32(g, gray_rs, (int)out_off, wave_uniform(v * (int)o.gray_stride), BUF_NT);
        us2 hsum;
        {   // horizontal [1 4 6 4 1] at the lane's two even columns c0 and c0+2
            const unsigned gl = up1(g), gr = down1(g);
            const unsigned a = dot4(alignb(g, gl, 2), 0x04060401u, byte_of(g, 2));
            const unsigned b = dot4(g, 0x04060401u, gr & 255u);
            hsum = as_us2(a | (b << 16));
        }
        if (PAR == 1 || (PAR == 0 && (v & 1))) {
            accA += hsum * (unsigned short)4;
            accB += hsum * (unsigned short)4;
            return;
        }
        us2 P = (accA + hsum) >> (unsigned short)8;
        accA = accB + hsum * (unsigned short)6;
        accB = hsum + (unsigned short)128;
        if (!S && v < v_first + 4) return;
        const int q = (v - 2) >> 1;  // pyramid row completed by source row 2q+2
        if (EDGE) P = as_us2(__builtin_amdgcn_perm(up1(as_u32(P)), as_u32(P), selP));   // pyrUp right border: column pw stands for column pw-1
        if (!S && q == ph_) P = as_us2(prevP);       // pyrUp bottom border: row ph stands for row ph-1
        else if (!S && q < ph_) prevP = as_u32(P);   // (steady rows end before source row sh-2: generic rows with q < ph follow them and set it)
        unsigned rCe, rCo;
        {   // horizontal up-sampling at the lane's 4 columns: even (r0,r2) and odd (r1,r3)
            const unsigned pk = as_u32(P);
            const us2 Lv = as_us2(alignb(pk, up1(pk), 2));     // (P[k0-1], P[k0])
            const us2 Rv = as_us2(alignb(down1(pk), pk, 2));   // (P[k0+1], P[k0+2])
            rCe = as_u32((Lv + P * (unsigned short)6 + Rv) << (unsigned short)2);
            rCo = as_u32((P + Rv) << (unsigned short)4);
        }
        if (S || q >= qa + 2) {
            for (int par = 0; par < 2; par++) {
                const int u = 2 * (q - 1) + par;
                if (!S && (u < 0 || u >= sh)) continue;
                us2 Ue, Uo;   // pyrUp row u at the lane's even columns (c0, c0+2) and odd columns (c0+1, c0+3)
                if (par == 0) {
                    Ue = Te + as_us2(rCe);
                    Uo = To + as_us2(rCo);
                } else {   // 4 (b - 128 + r) + 128 = 4 (b + r) - 384 (mod 2^16)
                    Ue = (be + as_us2(rCe)) * (unsigned short)4 + (unsigned short)(65536 - 384);
                    Uo = (bo + as_us2(rCo)) * (unsigned short)4 + (unsigned short)(65536 - 384);
                }
                // rows above 0 / below sh-1 replicate row 0 / sh-1; one more virtual row flushes the last mask row
                const int vlo = (!S && u == 0) ? -3 : u, vhi = (!S && u == sh - 1) ? sh + 3 : u;
                for (int vu = vlo; vu <= vhi; vu++) {
                    const int slot = VM >= 0 ? ((VM + par) & 3) : (vu & 3);   // steady rows: vu = u = v - 4 + par
                    if (slot == 0) {   // a new group of four rows: the words change names
                        if constexpr (VM >= 0) {
#pragma unroll
                            for (int p = 0; p < 4; p++) asm("v_swap_b32 %0, %1" : "+v"(wa[p]), "+v"(wb[p]));
                        } else {
#pragma unroll
                            for (int p = 0; p < 4; p++) { const unsigned t = wa[p]; wa[p] = wb[p]; wb[p] = t; }
                        }
                    }
                    {   // pixel p of the new row (u0, u2 = bytes 1, 3 of Ue -- the high bytes of its halves --; u1, u3 of Uo) into byte `slot` of wa[p]
                        const unsigned kb = 8u * (unsigned)slot, keep = 0x03020100u & ~(0xffu << kb);
                        const unsigned s4 = keep | (5u << kb), s6 = keep | (7u << kb);
                        wa[0] = __builtin_amdgcn_perm(as_u32(Ue), wa[0], s4);
                        wa[1] = __builtin_amdgcn_perm(as_u32(Uo), wa[1], s4);
                        wa[2] = __builtin_amdgcn_perm(as_u32(Ue), wa[2], s6);
                        wa[3] = __builtin_amdgcn_perm(as_u32(Uo), wa[3], s6);
                    }
                    const int y = vu - 3;   // the ring now holds pyrUp rows y-3 .. y+3 (and row vu-7: weight 0)
                    if (!S && (y < Y0 - 1 || y > Y1 || y < 0)) continue;
                    unsigned nib = 0;
                    if (S || (y >= 1 && y <= sh - 2)) {
                        // 7x7 Gaussian, vertical pass first: [8 28 56 72 56 28 8] over rows y-3 .. y+3.  Seen as eight slots (wa's bytes,
                        // then wb's) with the newest row in slot 7 the weights would be 0 8 28 56 | 72 56 28 8; the newest row is in
                        // slot `slot` of wa: that word pair rotated by whole bytes.
                        // (<= 256*255: the sums fit 16 bits and are packed in pairs for the horizontal pass)
                        const unsigned long long KW = rotl64(0x081C3848381C0800ull, 8u * (unsigned)((slot + 1) & 7));
                        const unsigned kwa = (unsigned)KW, kwb = (unsigned)(KW >> 32);
                        unsigned V[4];
#pragma unroll
                        for (int p = 0; p < 4; p++) V[p] = dot4(wa[p], kwa, dot4(wb[p], kwb, 0u));
                        const us2 Va = as_us2(V[0] | (V[1] << 16));
                        us2 Vb = as_us2(V[2] | (V[3] << 16));
                        if (EDGE) Vb = as_us2(__builtin_amdgcn_perm(as_u32(Va), as_u32(Vb), selB));   // (columns sw, sw+1 of the lane that straddles the right edge)
                        // horizontal pass: 16-bit column sums of this lane (Va = V0 V1, Vb = V2 V3), the lane to the left (l) and to
                        // the right (r), two taps per v_dot2_u32_u16 -- with neighbouring columns paired every pixel's 7 taps are 4
                        // instructions.  The accumulator starts at the rounding constant minus 8<<16:
                        // src - mean > -8  <=>  sum + 32768 - (8<<16) < src<<16
                        us2 Val = as_us2(up1(as_u32(Va))), Vbl = as_us2(up1(as_u32(Vb)));     // V-4 V-3, V-2 V-1
                        us2 Var = as_us2(down1(as_u32(Va))), Vbr = as_us2(down1(as_u32(Vb))); // V4 V5, V6 V7
                        if (EDGE) {   // BORDER_REPLICATE: columns < 0 are column 0, columns >= sw are column sw-1 (selL, selR above)
                            Val = as_us2(__builtin_amdgcn_perm(as_u32(Va), as_u32(Val), selL));
                            Vbl = as_us2(__builtin_amdgcn_perm(as_u32(Va), as_u32(Vbl), selL));
                            Var = as_us2(__builtin_amdgcn_perm(as_u32(Vb), as_u32(Var), selR));
                            Vbr = as_us2(__builtin_amdgcn_perm(as_u32(Vb), as_u32(Vbr), selR));
                        }
                        const unsigned C0 = 32768u - (8u << 16);
                        const unsigned S0 = dot2(Val, K2(0, 8), dot2(Vbl, K2(28, 56), dot2(Va, K2(72, 56), dot2(Vb, K2(28, 8), C0))));
                        const unsigned S1 = dot2(Vbl, K2(8, 28), dot2(Va, K2(56, 72), dot2(Vb, K2(56, 28), dot2(Var, K2(8, 0), C0))));
                        const unsigned S2 = dot2(Vbl, K2(0, 8), dot2(Va, K2(28, 56), dot2(Vb, K2(72, 56), dot2(Var, K2(28, 8), C0))));
                        const unsigned S3 = dot2(Va, K2(8, 28), dot2(Vb, K2(56, 72), dot2(Var, K2(56, 28), dot2(Vbr, K2(8, 0), C0))));
                        // pyrUp row y itself -- slot (slot - 3) & 7 of the eight -- is the threshold's source; nib = 2 * nib + (S < src << 16),
                        // pixel 3 first: one compare and one add-with-carry per pixel
                        const int ts = (slot + 5) & 7;
                        if constexpr (VM >= 0) {
                            constexpr int TS = ((VM & 3) + 5) & 7;   // par = 0; par = 1 is the next slot
                            if (par == 0) {
                                first_bit<TS & 3>(nib, S3, TS < 4 ? wa[3] : wb[3]);
                                push_bit<TS & 3>(nib, S2, TS < 4 ? wa[2] : wb[2]);
                                push_bit<TS & 3>(nib, S1, TS < 4 ? wa[1] : wb[1]);
                                push_bit<TS & 3>(nib, S0, TS < 4 ? wa[0] : wb[0]);
                            } else {
                                constexpr int T1 = (TS + 1) & 7;
                                first_bit<T1 & 3>(nib, S3, T1 < 4 ? wa[3] : wb[3]);
                                push_bit<T1 & 3>(nib, S2, T1 < 4 ? wa[2] : wb[2]);
                                push_bit<T1 & 3>(nib, S1, T1 < 4 ? wa[1] : wb[1]);
                                push_bit<T1 & 3>(nib, S0, T1 < 4 ? wa[0] : wb[0]);
                            }
                        } else {
                            const unsigned tsel = 0x0c000c0cu | ((unsigned)ts << 16);   // byte ts of (wb : wa) into byte 2, zeros elsewhere
#define OCVAR_PUSH_BIT(S, P) asm("v_cmp_lt_i32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(nib) : "v"(S), "v"(__builtin_amdgcn_perm(wb[P], wa[P], tsel)) : "vcc")
                            OCVAR_PUSH_BIT(S3, 3);
                            OCVAR_PUSH_BIT(S2, 2);
                            OCVAR_PUSH_BIT(S1, 1);
                            OCVAR_PUSH_BIT(S0, 0);
#undef OCVAR_PUSH_BIT
                        }
                        if (EDGE || VM < 0) nib &= colmask;   // (strips inside the image: every column counts, and the four tests above left four bits)
                    }
                    // row y into the ring (here y >= max(Y0 - 1, 0) and y <= Y1); flush_due, between rows, makes tile rows of it
                    rowbuf[(y & (RING_ROWS - 1)) * 64 + lane] = (uint8_t)nib;
                    y_in = y;
                }
            }
        }
        Te = as_us2(rCe) * (unsigned short)6 + be;
        To = as_us2(rCo) * (unsigned short)6 + bo;
        be = as_us2(rCe) + (unsigned short)128;
        bo = as_us2(rCo) + (unsigned short)128;
    };
    // steady rows: v and v+1 are real rows of this unit ([Y0, Y1), v+1 <= sh-1), and the rows an even v completes -- pyrUp
    // rows v-4, v-3, threshold rows v-7, v-6, mask rows v-8, v-7 -- are inside the unit, at least one row away from the
    // image's top and bottom (no replicated pyrUp rows, no zeroed contour-frame rows) and not the unit's last mask row
    // -- and the unit has the load plan (else no row is steady: the steady instance of the row body does not carry the byte-wise
    // loads of images narrower than 32 columns)
    const bool steady_ok = plan;
    const int vs0 = (Y0 + 8 > 8 ? Y0 + 8 : 8) | 1, vs1 = !steady_ok ? -1 : Y1 - 1 < sh - 2 - AHEAD ? Y1 - 1 : sh - 2 - AHEAD;   // (vs0 odd: steady rows run in pairs; v + 2 is a real row: prefetched unreflected)
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    using P2 = std::integral_constant<int, 2>;
    using RX = std::integral_constant<int, -1>;   // ring position not known at compile time
    int v = v_first;
#pragma nounroll
    for (int phase = 0; phase < 2; phase++) {   // generic rows, steady rows, generic rows: one copy of each instance
        const int end = phase == 0 ? (vs0 <= v_last + 1 ? vs0 : v_last + 1) : v_last + 1;
        for (; v < end; v++) {
            row(v, std::false_type(), P0(), RX());
            flush_due();
        }
        if (phase == 0)
            while (v + 1 <= vs1) {
                if ((v & 3) == 1 && v + 3 <= vs1) {   // four rows with the ring's position known: the hot loop
                    row(v, std::true_type(), P1(), RX());
                    row(v + 1, std::true_type(), P2(), std::integral_constant<int, 2>());
                    row(v + 2, std::true_type(), P1(), RX());
                    row(v + 3, std::true_type(), P2(), std::integral_constant<int, 0>());
                    v += 4;
                    flush_due();
                } else {                               // a pair before the first or after the last group of four
                    row(v, std::true_type(), P1(), RX());
                    row(v + 1, std::true_type(), P2(), RX());
                    v += 2;
                    flush_due();
                }
            }
    }
    flush();
}

// Workgroups of ONE wave (BW = 1): the waves of a workgroup must be placed on their CU together, so a four-wave workgroup needs
// room on all four SIMDs at once -- and with other contexts' kernels on the GPU (a follower wave of 110 registers on one SIMD)
// a CU holds a whole workgroup less.  A one-wave workgroup takes any SIMD with 96 free registers and 4 KB of LDS.
constexpr int BW = OCVAR_BIN_WG_WAVES;

// One instance per source format (FMT: OCVAR_FMT_*); they differ in the row loads and the grey conversion only.
template <int FMT>
__global__ __launch_bounds__(64 * BW) __attribute__((amdgpu_waves_per_eu(OCVAR_WAVES_F, 8))) void binarise_frames_kernel(Workspace ws, const uint8_t* bgr, int row_stride, size_t frame_stride) {
    __shared__ unsigned stage[BW][MARCH_STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t rowbuf[BW][RING_ROWS * 64];
    const int per_frame = ws.frame_strips * ws.frame_chunks;
    // XCD-aware order.  Consecutive workgroups go round the 8 XCDs, each with its own L2; in launch order the workgroups of one
    // frame -- neighbouring strips and chunks, which share halo columns and rows -- would land on 8 different L2s and every halo
    // would be fetched from the fabric twice.  Workgroup b therefore works on frame-group (b / 8) / G, frame b % 8 of that group,
    // workgroup (b / 8) % G of that frame (G workgroups per frame): a frame's workgroups run on one XCD, next to each other in
    // time.  (Only when a frame is a whole number of workgroups; the frames beyond the last group of 8 keep launch order.)
    int wg = (int)blockIdx.x;
    if (per_frame % BW == 0) {
        const int G = per_frame / BW, grouped = (ws.n_frames & ~7) * G;
        if (wg < grouped) {
            const int k = wg >> 3;
            wg = ((k / G) * 8 + (wg & 7)) * G + k % G;
        }
    }
    const int unit = wg * BW + wave_uniform((int)(threadIdx.x >> 6));
    if (unit >= per_frame * ws.n_frames) return;
    const int f = unit / per_frame, rem = unit % per_frame;
    const int chunk = rem / ws.frame_strips, strip = rem % ws.frame_strips;
    const int Y0 = chunk * ws.frame_chunk_rows;
    const int Y1 = Y0 + ws.frame_chunk_rows < ws.sh ? Y0 + ws.frame_chunk_rows : ws.sh;
    MarchOut o;
    o.gray = ws.gray + (size_t)f * gray_plane_bytes(ws.W, ws.H);
    o.gray_stride = gray_pitch(ws.W);
    o.nbr = ws.nbr_frame + (size_t)f * nbr_plane_bytes(ws.ns, ws.sh);
    o.ns = ws.ns;
    o.roi = f;
    o.cands = ws.cands_frame;
    o.n_cands = ws.counters + CNT_FRAME_CANDS;
    o.cap_cands = ws.cap_frame_cands;
    o.err = ws.counters + CNT_ERR;
    const int w4 = wave_uniform((int)(threadIdx.x >> 6));
    const bool edge = strip == 0 || ((ws.sw - 1 - (strip * MARCH_STRIP - 4 * MARCH_HALO_L)) >> 2) <= 63;   // march_unit's left_edge || right_edge
    if (edge) march_unit<FMT, true>(bgr + (size_t)f * frame_stride, row_stride, 0, ws.sw, ws.sh, strip, Y0, Y1, o, stage[w4], rowbuf[w4]);
    else march_unit<FMT, false>(bgr + (size_t)f * frame_stride, row_stride, 0, ws.sw, ws.sh, strip, Y0, Y1, o, stage[w4], rowbuf[w4]);
}

// grey of the source pixel at p in format fmt (OCVAR_FMT_*)
__device__ __forceinline__ uint8_t grey_at(const uint8_t* p, int fmt) {
    if (fmt == OCVAR_FMT_GRAY) return p[0];
    const bool rev = fmt == OCVAR_FMT_RGB || fmt == OCVAR_FMT_RGBA;
    return (uint8_t)grey_of(p[rev ? 2 : 0], p[1], p[rev ? 0 : 2]);
}

// Odd width / height: the last column / row lies outside the even working size (opencvar.cpp:158) but is still
// greyed by cvarArMultRegistration's BGR2GRAY.
__global__ __launch_bounds__(256) void grey_edges_kernel(Workspace ws, const uint8_t* bgr, int row_stride, size_t frame_stride, int fmt) {
    const int f = blockIdx.y;
    const uint8_t* src = bgr + (size_t)f * frame_stride;
    uint8_t* g = ws.gray + (size_t)f * gray_plane_bytes(ws.W, ws.H);
    const int pitch = gray_pitch(ws.W);
    const int n_col = ws.W > ws.sw ? ws.H : 0, n_row = ws.H > ws.sh ? ws.W : 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_col + n_row; i += gridDim.x * blockDim.x) {
        const int x = i < n_col ? ws.sw : i - n_col, y = i < n_col ? i : ws.sh;
        const uint8_t* p = src + (long long)y * row_stride + src_bpp(fmt) * x;
        const uint8_t v = grey_at(p, fmt);
        g[(long long)y * pitch + gray_col(x)] = v;
        // (a column within 8 of a panel's start is also kept at the end of the panel before: readers take the panel of a run's first column)
        if (x >= GRAY_PANEL_COLS && x % GRAY_PANEL_COLS < GRAY_PANEL_LEAD) g[(long long)y * pitch + gray_col(x - GRAY_PANEL_LEAD) + GRAY_PANEL_LEAD] = v;
    }
}

// The reference greys the caller's frame in place (opencvar.cpp:624-627).  Done as its own pass over the
// grey plane so that no wave ever reads a half-written BGR pixel of a neighbouring strip's halo.  Bytes 0..2 of a pixel take
// the grey value, a four-channel pixel's byte 3 is left as it is; a grey frame is its own grey (not launched).
__global__ __launch_bounds__(256) void grey_writeback_kernel(Workspace ws, uint8_t* bgr, int row_stride, size_t frame_stride, int bpp) {
    const int f = blockIdx.y;
    const uint8_t* g = ws.gray + (size_t)f * gray_plane_bytes(ws.W, ws.H);
    const int pitch = gray_pitch(ws.W);
    uint8_t* dst = bgr + (size_t)f * frame_stride;
    const long long n = (long long)ws.W * ws.H;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % ws.W), y = (int)(i / ws.W);
        const uint8_t v = g[(long long)y * pitch + gray_col(x)];
        uint8_t* q = dst + (long long)y * row_stride + bpp * x;
        q[0] = q[1] = q[2] = v;
    }
}

__global__ __launch_bounds__(64 * BW) __attribute__((amdgpu_waves_per_eu(OCVAR_WAVES_C, 8))) void binarise_crops_kernel(Workspace ws) {
    __shared__ unsigned stage[BW][MARCH_STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t rowbuf[BW][RING_ROWS * 64];
    int n_units = ws.counters[CNT_CROP_TILES];
    if (n_units > ws.cap_crop_tiles) n_units = ws.cap_crop_tiles;
    const int wave = wave_uniform((int)(threadIdx.x >> 6));
    // crop units differ in size (rows, and the follow-up of their start lists): waves pull them from a ticket counter.
    // (The ticket test uses an opaque copy of the lane id: see follow.hip::ticket_lane for the compiler hazard.)
    int* ticket = ws.counters + CNT_TICKET_BC;
    // a wave can be handed at most n_units tickets (+ the one that tells it to stop): anything beyond that means the loop's
    // control flow is broken; report instead of spinning
    for (int guard = n_units + 1;; guard--) {
        if (guard < 0) {
            if ((threadIdx.x & 63) == 0) atomicOr(ws.counters + CNT_ERR, ERR_TICKET_RUNAWAY);
            break;
        }
        int lane_id = (int)(threadIdx.x & 63);
        asm volatile("" : "+v"(lane_id));
        int u = 0;
        if (lane_id == 0) u = atomicAdd(ticket, 1);
        u = wave_uniform(u);
        if (u >= n_units) break;
        const TileDesc td = ws.tiles_crop[u];
        const Roi r = ws.rois_crop[td.roi];
        const int pitch = gray_pitch(ws.W);
        const uint8_t* src = ws.gray + (size_t)r.frame * gray_plane_bytes(ws.W, ws.H) + (size_t)r.y0 * pitch;   // (row y0 of the frame's panelled grey plane; the columns go through gray_col(r.x0 + column))
        const int Y1 = td.y0 + MARCH_CROP_ROWS < r.sh ? td.y0 + MARCH_CROP_ROWS : r.sh;
        MarchOut o;
        o.gray = nullptr;
        o.gray_stride = 0;
        o.nbr = ws.nbr_crop + r.nbr_off;
        o.ns = r.ns;
        o.roi = td.roi;
        o.cands = ws.cands_crop;
        o.n_cands = ws.counters + CNT_CROP_CANDS;
        o.cap_cands = ws.cap_crop_cands;
        o.err = ws.counters + CNT_ERR;
        march_unit<SRC_CROP, true>(src, pitch, r.x0, r.sw, r.sh, td.x0, td.y0, Y1, o, stage[wave], rowbuf[wave]);
    }
}

void launch_binarise_frames(const Workspace& ws, const uint8_t* d_bgr, int row_stride, size_t frame_stride, int grey_in_place,
                            int format, hipStream_t stream) {
    const int units = ws.frame_strips * ws.frame_chunks * ws.n_frames;
    if (units <= 0) return;
    const dim3 grid((units + BW - 1) / BW), block(64 * BW);
    switch (format) {
    case OCVAR_FMT_RGB: hipLaunchKernelGGL(binarise_frames_kernel<OCVAR_FMT_RGB>, grid, block, 0, stream, ws, d_bgr, row_stride, frame_stride); break;
    case OCVAR_FMT_BGRA: hipLaunchKernelGGL(binarise_frames_kernel<OCVAR_FMT_BGRA>, grid, block, 0, stream, ws, d_bgr, row_stride, frame_stride); break;
    case OCVAR_FMT_RGBA: hipLaunchKernelGGL(binarise_frames_kernel<OCVAR_FMT_RGBA>, grid, block, 0, stream, ws, d_bgr, row_stride, frame_stride); break;
    case OCVAR_FMT_GRAY: hipLaunchKernelGGL(binarise_frames_kernel<OCVAR_FMT_GRAY>, grid, block, 0, stream, ws, d_bgr, row_stride, frame_stride); break;
    default: hipLaunchKernelGGL(binarise_frames_kernel<OCVAR_FMT_BGR>, grid, block, 0, stream, ws, d_bgr, row_stride, frame_stride); break;
    }
    if (ws.W > ws.sw || ws.H > ws.sh)
        hipLaunchKernelGGL(grey_edges_kernel, dim3(8, ws.n_frames), dim3(256), 0, stream, ws, d_bgr, row_stride, frame_stride, format);
    if (grey_in_place && format != OCVAR_FMT_GRAY)
        hipLaunchKernelGGL(grey_writeback_kernel, dim3(1024, ws.n_frames), dim3(256), 0, stream, ws, const_cast<uint8_t*>(d_bgr),
                           row_stride, frame_stride, src_bpp(format));
}

void launch_binarise_crops(const Workspace& ws, hipStream_t stream) {
    hipLaunchKernelGGL(binarise_crops_kernel, dim3(ws.crop_blocks * (4 / BW)), dim3(64 * BW), 0, stream, ws);   // (crop_blocks counts four waves each)
}

}  // namespace ocvar
