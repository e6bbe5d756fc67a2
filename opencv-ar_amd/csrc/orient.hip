// orient.hip -- opt-in turning and mirroring of device-resident frames and of marker records (ocvar_hip_orient /
// ocvar_hip_orient_records).  The definition is orient_core.h's; its host build (tests/emul/orient_emul.cpp) gives these kernels'
// bytes.  A pure permutation of pixels: no workspace, the arguments travel by value, the kernels are templates of the bytes per
// pixel and the alignment, not of the sizes.  Three classes:
//
//   rows kept      IDENTITY, FLIP_V.  A one-wave workgroup owns a span of ORIENT_WAVE_PX pixels of one destination row (blockIdx:
//                  span, row, frame; at 1 byte per pixel of 4 consecutive rows, one after the other), a lane ORIENT_LANE_PX
//                  consecutive ones: it loads the same run of source row y or H - 1 - y and stores it, 2 BPP whole dwords each
//                  way.
//   rows reversed  FLIP_H, ROT180.  The same ownership; the lane's source is the mirrored contiguous run, loaded as whole dwords
//                  when its address is a multiple of 4 (address and strides are, and BPP W is), reversed in registers -- a byte
//                  swap (v_perm_b32) of the two dwords at 1 byte per pixel, the dwords in reverse order at 4, a fixed shuffle of
//                  the 24 bytes over 6 dwords at 3 -- and stored as whole dwords.
//   transposing    ROT90_CW, ROT270_CW, TRANSPOSE, TRANSVERSE.  A workgroup of 4 waves moves one tile of ORIENT_TILE x ORIENT_TILE
//                  pixels through LDS (blockIdx: tile along destination x, tile along source x, frame).  Tiles are anchored at
//                  destination x = 0 and at source x = 0, the two axes along which bytes are contiguous, so a tile's first byte
//                  is a multiple of 4 on both sides whatever the sizes are, and partial tiles lie at the far ends only; the two
//                  reversals are absorbed where they cost nothing: which source ROW goes to LDS row u, and which destination ROW
//                  LDS column c is stored to.  What happens in LDS is always the plain transposition.
//                    load   source row segments of 64 pixels = 64 BPP contiguous bytes as whole dwords, consecutive lanes on
//                           consecutive dwords (64, 192 or 256 contiguous bytes per segment, one to four segments per wave
//                           instruction), written with ds_write_b32 to LDS row u: the segment of the source row that becomes
//                           destination column dx0 + u.
//                    read   a lane assembles ORIENT_TILE_RUN = 4 consecutive destination pixels of one destination row: column
//                           c of LDS rows u0 .. u0 + 3.  1 byte per pixel: four ds_read_b32 of the dword that holds columns
//                           4 cb .. 4 cb + 3, a 4 x 4 byte transposition with 8 v_perm_b32, four dword stores to four destination
//                           rows.  4 bytes: four ds_read_b32, one 16-byte run.  3 bytes: twelve ds_read_u8, one 12-byte run.
//                    store  consecutive lanes own consecutive runs of one destination row: 64, 192 or 256 contiguous bytes per
//                           row per 16 lanes, whole dwords.
//                  LDS geometry: an image row holds DPR = 16 BPP dwords at a pitch of PITCH = DPR + 9 dwords (PITCH = 1 mod 8),
//                  and rows 32 .. 63 are shifted by 2 dwords: dword j of row u is word u PITCH + j + 2 (u >> 5).
//                  Conflict argument (ds_read_b32 / ds_read_u8: bank = dword address mod 32, the lanes of one 32-lane half
//                  conflict): a half-wave reads, for one k, rows u = 4 rb + k, rb = 0 .. 15, at two neighbouring columns.
//                  u PITCH = 4 rb PITCH + k PITCH = 4 rb + const (mod 32) because 4 PITCH = 4 (mod 32); 4 rb mod 32 takes 8 values,
//                  each for rb and rb + 8, and rb + 8 is a row of the shifted half: banks 4 rb + {0, 1} for rb < 8 and
//                  4 (rb - 8) + {2, 3} for rb >= 8 (plus the constant) -- 32 distinct banks, conflict-free.  At 3 bytes per pixel
//                  the two columns' bytes lie in the same dword (one address: a broadcast) or in neighbouring ones: the same
//                  argument.  The writes put consecutive lanes on consecutive words of a row; a wave instruction that spans
//                  several rows (1 byte per pixel: 4 rows of 16 dwords) overlaps by the pitch's odd dword, 2-way on ds_write_b32,
//                  which costs nothing.
//
// All classes: with ALIGNED (every address, row stride and frame stride on both sides a multiple of 4) full runs move as whole
// dwords; the last pixels of a row or tile, and everything when something is unaligned, move byte by byte with the same result
// and touch nothing past their pixels.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int ORIENT_LANE_PX = 8;                       // consecutive destination pixels of one row a lane of the row kernels owns
constexpr int ORIENT_WAVE_PX = 64 * ORIENT_LANE_PX;     // destination pixels of one wave's span
constexpr int ORIENT_TILE = 64;                         // pixels of a tile's side
constexpr int ORIENT_TILE_RUN = 4;                      // consecutive destination pixels a lane of the tile kernel assembles
constexpr int ORIENT_TILE_THREADS = 256;
constexpr int ORIENT_RUNS = ORIENT_TILE / ORIENT_TILE_RUN;   // runs per destination row of a tile

// byte i of the result is byte sel[i] of the eight bytes lo (0 .. 3), hi (4 .. 7): v_perm_b32
OCVAR_D unsigned byte_perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// The ORIENT_LANE_PX pixels of w in reverse order.
template <int BPP>
OCVAR_D void reverse_run(const unsigned (&w)[2 * BPP], unsigned (&q)[2 * BPP]) {
    if constexpr (BPP == 1) {
        q[0] = byte_perm(0u, w[1], 0x00010203u);
        q[1] = byte_perm(0u, w[0], 0x00010203u);
    } else if constexpr (BPP == 4) {
        OCVAR_UNROLL
        for (int i = 0; i < ORIENT_LANE_PX; i++) q[i] = w[ORIENT_LANE_PX - 1 - i];
    } else {   // constant indices: a fixed shuffle of 24 bytes
        OCVAR_UNROLL
        for (int j = 0; j < 2 * BPP; j++) q[j] = 0;
        OCVAR_UNROLL
        for (int i = 0; i < ORIENT_LANE_PX; i++) {
            OCVAR_UNROLL
            for (int c = 0; c < BPP; c++) run_put(q, i * BPP + c, run_byte(w, (ORIENT_LANE_PX - 1 - i) * BPP + c));
        }
    }
}

// Rows kept (REV false) and rows reversed (REV true); flip_rows: destination row y is source row H - 1 - y.  A workgroup takes
// its span in orient_rows(BPP) consecutive destination rows, all loads first: at 1 byte per pixel a wave that moved one row's 512
// bytes reached 0.40 of a plain copy's rate (1920x1080 FLIP_H, 32 frames), too little in flight per wave.
constexpr int orient_rows(int bpp) { return bpp == 1 ? 4 : 1; }
template <int BPP, bool ALIGNED, bool REV>
__global__ __launch_bounds__(64) void orient_rows_kernel(OrientArgs a, int flip_rows) {
    constexpr int ROWS = orient_rows(BPP);
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * ORIENT_LANE_PX;
    if (x0 >= a.sw) return;
    const int y0 = (int)blockIdx.y * ROWS;
    const int npx = a.sw - x0 < ORIENT_LANE_PX ? a.sw - x0 : ORIENT_LANE_PX;
    const bool dwords = ALIGNED && npx == ORIENT_LANE_PX;
    const uint8_t* src = a.src + (long long)blockIdx.z * a.src_frame_stride;
    uint8_t* out = a.dst + (long long)blockIdx.z * a.dst_frame_stride + (long long)x0 * BPP;
    // REV: the source run is pixels W - x0 - 8 .. W - x0 - 1; of the row's last lane the first 8 - npx lie before the row and are
    // neither read nor stored
    const long long s0 = REV ? ((long long)a.sw - x0 - ORIENT_LANE_PX) * BPP : (long long)x0 * BPP;
    unsigned w[ROWS][2 * BPP];
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) {
        const int y = y0 + r;
        if (y >= a.sh) break;
        const uint8_t* row = src + (long long)(flip_rows ? a.sh - 1 - y : y) * a.src_row_stride;
        if (!REV) {
            run_load(w[r], row + s0, dwords, npx * BPP);
        } else if (dwords && (s0 & 3) == 0) {
            run_load(w[r], row + s0, true, ORIENT_LANE_PX * BPP);
        } else {
            const int lead = (ORIENT_LANE_PX - npx) * BPP;
            OCVAR_UNROLL
            for (int j = 0; j < 2 * BPP; j++) w[r][j] = 0;
            OCVAR_UNROLL
            for (int b = 0; b < ORIENT_LANE_PX * BPP; b++)
                if (b >= lead) w[r][b >> 2] |= (unsigned)row[s0 + b] << (8 * (b & 3));
        }
    }
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) {
        const int y = y0 + r;
        if (y >= a.sh) break;
        unsigned q[2 * BPP];
        if (REV) {
            reverse_run<BPP>(w[r], q);
        } else {
            OCVAR_UNROLL
            for (int j = 0; j < 2 * BPP; j++) q[j] = w[r][j];
        }
        run_store(q, out + (long long)y * a.dst_row_stride, dwords, npx * BPP);
    }
}

// dwords of a tile row of the LDS image, its pitch, and the word of dword j of row u
template <int BPP>
struct OrientTile {
    static constexpr int DPR = ORIENT_TILE * BPP / 4, PITCH = DPR + 9, WORDS = ORIENT_TILE * PITCH;
    static_assert(PITCH % 8 == 1, "the conflict argument at the top of the file");
    static OCVAR_D int at(int u, int j) { return u * PITCH + j + 2 * (u >> 5); }
};

// The transposing class; dw = a.sh is the destination's width.  rev_x: destination column dx is source row H - 1 - dx, not dx;
// rev_y: source column sx goes to destination row W - 1 - sx, not sx.
template <int BPP, bool ALIGNED>
__global__ __launch_bounds__(ORIENT_TILE_THREADS) void orient_tile_kernel(OrientArgs a, int rev_x, int rev_y) {
    using T = OrientTile<BPP>;
    __shared__ unsigned img[T::WORDS];
    const int tid = threadIdx.x;
    const int dx0 = (int)blockIdx.x * ORIENT_TILE, sx0 = (int)blockIdx.y * ORIENT_TILE;
    const int nu = a.sh - dx0 < ORIENT_TILE ? a.sh - dx0 : ORIENT_TILE;      // destination columns = LDS rows of this tile
    const int nc = a.sw - sx0 < ORIENT_TILE ? a.sw - sx0 : ORIENT_TILE;      // source columns = LDS columns of this tile
    const uint8_t* src = a.src + (long long)blockIdx.z * a.src_frame_stride + (long long)sx0 * BPP;
    uint8_t* dst = a.dst + (long long)blockIdx.z * a.dst_frame_stride + (long long)dx0 * BPP;
    const int row_bytes = nc * BPP;
    // every lane's dwords of the tile are loaded before the first is written to LDS: 4 BPP loads in flight per lane
    constexpr int LOADS = ORIENT_TILE * T::DPR / ORIENT_TILE_THREADS;
    static_assert(LOADS * ORIENT_TILE_THREADS == ORIENT_TILE * T::DPR, "whole rounds");
    unsigned v[LOADS];
    OCVAR_UNROLL
    for (int k = 0; k < LOADS; k++) {
        const int i = tid + k * ORIENT_TILE_THREADS, u = i / T::DPR, j = i - u * T::DPR;
        v[k] = 0;
        if (u < nu && 4 * j < row_bytes) {
            const uint8_t* p = src + (long long)(rev_x ? a.sh - 1 - (dx0 + u) : dx0 + u) * a.src_row_stride + 4 * j;
            if (ALIGNED && 4 * j + 4 <= row_bytes) {
                v[k] = *reinterpret_cast<const unsigned*>(p);
            } else {
                OCVAR_UNROLL
                for (int b = 0; b < 4; b++)
                    if (4 * j + b < row_bytes) v[k] |= (unsigned)p[b] << (8 * b);
            }
        }
    }
    OCVAR_UNROLL
    for (int k = 0; k < LOADS; k++) {      // (words of rows and columns beyond the frame get 0: nothing reads them)
        const int i = tid + k * ORIENT_TILE_THREADS, u = i / T::DPR;
        img[T::at(u, i - u * T::DPR)] = v[k];
    }
    __syncthreads();
    if constexpr (BPP == 1) {
        // one 4 x 4 block of bytes per lane: LDS rows u0 .. u0 + 3 at dword cb -> destination rows of columns 4 cb .. 4 cb + 3
        const int u0 = (tid & (ORIENT_RUNS - 1)) * ORIENT_TILE_RUN, cb = tid / ORIENT_RUNS;
        if (u0 >= nu || 4 * cb >= nc) return;
        const unsigned r0 = img[T::at(u0, cb)], r1 = img[T::at(u0 + 1, cb)], r2 = img[T::at(u0 + 2, cb)], r3 = img[T::at(u0 + 3, cb)];
        const unsigned t0 = byte_perm(r1, r0, 0x05010400u), t1 = byte_perm(r1, r0, 0x07030602u);   // r0.0 r1.0 r0.1 r1.1 | r0.2 r1.2 r0.3 r1.3
        const unsigned t2 = byte_perm(r3, r2, 0x05010400u), t3 = byte_perm(r3, r2, 0x07030602u);
        const unsigned o[4] = {byte_perm(t2, t0, 0x05040100u), byte_perm(t2, t0, 0x07060302u), byte_perm(t3, t1, 0x05040100u),
                               byte_perm(t3, t1, 0x07060302u)};                                    // o[c]: byte c of r0 r1 r2 r3
        const int n = nu - u0 < ORIENT_TILE_RUN ? nu - u0 : ORIENT_TILE_RUN;
        OCVAR_UNROLL
        for (int c = 0; c < 4; c++) {
            const int sx = sx0 + 4 * cb + c;
            if (sx < a.sw) {
                const unsigned q[1] = {o[c]};
                run_store(q, dst + (long long)(rev_y ? a.sw - 1 - sx : sx) * a.dst_row_stride + u0, ALIGNED && n == ORIENT_TILE_RUN, n);
            }
        }
    } else {
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(img);
        OCVAR_UNROLL
        for (int i = tid; i < ORIENT_TILE * ORIENT_RUNS; i += ORIENT_TILE_THREADS) {
            const int u0 = (i & (ORIENT_RUNS - 1)) * ORIENT_TILE_RUN, c = i / ORIENT_RUNS;
            if (u0 >= nu || c >= nc) continue;
            unsigned q[BPP];
            OCVAR_UNROLL
            for (int j = 0; j < BPP; j++) q[j] = 0;
            OCVAR_UNROLL
            for (int k = 0; k < ORIENT_TILE_RUN; k++) {
                if constexpr (BPP == 4) {
                    q[k] = img[T::at(u0 + k, c)];
                } else {
                    OCVAR_UNROLL
                    for (int ch = 0; ch < BPP; ch++) run_put(q, k * BPP + ch, bytes[4 * T::at(u0 + k, 0) + c * BPP + ch]);
                }
            }
            const int n = nu - u0 < ORIENT_TILE_RUN ? nu - u0 : ORIENT_TILE_RUN;
            const int sx = sx0 + c;
            run_store(q, dst + (long long)(rev_y ? a.sw - 1 - sx : sx) * a.dst_row_stride + (long long)u0 * BPP, ALIGNED && n == ORIENT_TILE_RUN,
                      n * BPP);
        }
    }
}

template <int BPP, bool ALIGNED>
static void launch_aligned(const OrientArgs& a, int n_frames, hipStream_t stream) {
    const int o = a.orientation;
    if (orient_transposes(o)) {
        const dim3 grid((a.sh + ORIENT_TILE - 1) / ORIENT_TILE, (a.sw + ORIENT_TILE - 1) / ORIENT_TILE, n_frames);
        hipLaunchKernelGGL((orient_tile_kernel<BPP, ALIGNED>), grid, dim3(ORIENT_TILE_THREADS), 0, stream, a, (int)orient_reverses_x(o),
                           (int)orient_reverses_y(o));
        return;
    }
    const dim3 grid((a.sw + ORIENT_WAVE_PX - 1) / ORIENT_WAVE_PX, (a.sh + orient_rows(BPP) - 1) / orient_rows(BPP), n_frames);
    if (orient_reverses_x(o)) hipLaunchKernelGGL((orient_rows_kernel<BPP, ALIGNED, true>), grid, dim3(64), 0, stream, a, (int)orient_reverses_y(o));
    else hipLaunchKernelGGL((orient_rows_kernel<BPP, ALIGNED, false>), grid, dim3(64), 0, stream, a, (int)orient_reverses_y(o));
}

template <int BPP>
static void launch_bpp(const OrientArgs& a, int n_frames, hipStream_t stream) {
    if (frames_dwords(a.src, a.src_row_stride, a.src_frame_stride) && frames_dwords(a.dst, a.dst_row_stride, a.dst_frame_stride)) launch_aligned<BPP, true>(a, n_frames, stream);
    else launch_aligned<BPP, false>(a, n_frames, stream);
}

void launch_orient(const OrientArgs& a, int n_frames, int format, hipStream_t stream) {
    if (n_frames <= 0 || a.sw <= 0 || a.sh <= 0 || !orient_ok(a.orientation)) return;
    switch (format_bpp(format)) {
        case 1: launch_bpp<1>(a, n_frames, stream); break;
        case 3: launch_bpp<3>(a, n_frames, stream); break;
        case 4: launch_bpp<4>(a, n_frames, stream); break;
        default: break;
    }
}

// One lane per record slot k < min(count, slots) of every frame (blockIdx: 64 slots, frame); the other slots are not written.
// A lane reads its record before it writes it, so out may be in.
__global__ __launch_bounds__(64) void orient_records_kernel(OrientRecArgs a) {
    const int k = (int)blockIdx.x * 64 + (int)threadIdx.x, f = blockIdx.y;
    int n = a.counts[f];
    n = n < a.slots ? n : a.slots;
    if (k >= n) return;
    MarkerRec r = a.in[(size_t)f * a.slots + k];
    orient_record(r, a.sw, a.sh, a.orientation, a.flags, a.cam);
    a.out[(size_t)f * a.slots + k] = r;
}

void launch_orient_records(const OrientRecArgs& a, int n_frames, hipStream_t stream) {
    if (n_frames <= 0 || a.slots <= 0) return;
    hipLaunchKernelGGL(orient_records_kernel, dim3((a.slots + 63) / 64, n_frames), dim3(64), 0, stream, a);
}

}  // namespace ocvar
