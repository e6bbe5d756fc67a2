// warp.hip -- opt-in projective warp of device-resident frames, of marker records, and the maps of a board's plane (ocvar_hip_warp /
// ocvar_hip_warp_records / ocvar_hip_board_plane_maps).  The definition is warp_core.h's; its host build (tests/emul/warp_emul.cpp)
// gives these kernels' bytes.  No workspace: the maps are read from the caller's device memory, everything else travels by value.
//
// warp_kernel: a workgroup of WARP_THREADS = 256 lanes owns a destination tile of WARP_TILE_W x warp_tile_h(bpp) pixels -- 64 x 64
// at 1 byte per pixel, 64 x 32 at 3 and 4 -- (blockIdx: tile column, tile row, frame).  A lane owns WARP_LANE_PX = 4 consecutive
// pixels of one row -- 4, 12 or 16 bytes, put together in registers and stored as whole dwords (ALIGNED: the destination's address,
// row stride and frame stride are multiples of 4) except in the lane that crosses the row's end; everything else goes byte by
// byte: undistort_kernel's ownership -- in warp_lane_rows(bpp) = 4 or 2 rows WARP_ROW_STEP = 16 apart, one after the other.
// Lane 0 inverts the frame's map and computes the tile's plan (warp_tile_plan) once for the workgroup and hands both over in LDS.
//   staged   the plan's source window goes to LDS first: its dwords, row after row from the dword that holds a row's first window
//            byte, are dealt to the 256 lanes in turn, consecutive lanes on consecutive dwords, four per lane in flight (row and
//            column of a dword by a multiplication with the row length's reciprocal, which lane 0 hands over too) -- whole-dword
//            loads when the source's address and strides are multiples of 4 and the dword ends inside the row's pixels, else the
//            bytes inside the row's pixels one by one (never a byte past them).  The image's pitch is odd (rows of a wave's four
//            destination rows start in different banks) and has a spare dword.
//            LINEAR pixels whose four taps lie in the window -- all of them unless the plan's margin was too small -- read, per
//            source row, the 2 (1 and 4 bytes per pixel) or 3 (3 bytes) aligned dwords that hold the two neighbouring source
//            pixels (ds_read_b32) and shift the pixels out of them (v_alignbyte_b32): 4 or 6 LDS reads per pixel in place of the
//            direct class's 4, 12 or 16 byte loads from global memory.  Every other pixel (NEAREST, taps on the border or beyond
//            the window) goes through the core's sampler tap by tap, each tap from LDS when the window holds it and from global
//            memory when not: the bytes never depend on the plan.
//   direct   no staging, every tap a byte load from global memory through the core's sampler: the shape of undistort_kernel.  Tiles
//            the horizon crosses, tiles whose window is too large (strong shrinking), and every tile under OCVAR_TUNE_WARP_DIRECT.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

static_assert(WARP_TILE_W * WARP_ROW_STEP == WARP_THREADS * WARP_LANE_PX && WARP_TILE_W % WARP_LANE_PX == 0, "a lane owns one run in each of its tile rows");

constexpr int WARP_STAGE_LOADS = 4;     // dwords of the window a lane loads before it writes the first to LDS

// what lane 0 hands to the workgroup; recip: ceil(2^32 / plan.row_dwords), with which i / row_dwords is the high dword of
// i * recip for every i below the image's 4096 dwords (i * row_dwords < 2^32; a row of 1 dword needs none)
struct WarpTile {
    double M[9];
    WarpPlan plan;
    unsigned recip;
    int ok;
};

// bytes s .. s + 3 of the eight bytes lo (0 .. 3), hi (4 .. 7), s = 0 .. 3: v_alignbyte_b32
OCVAR_D unsigned align_bytes(unsigned hi, unsigned lo, int s) { return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)s); }

template <int BPP, bool ALIGNED>
__global__ __launch_bounds__(WARP_THREADS) void warp_kernel(WarpArgs a) {
    constexpr int TILE_H = warp_tile_h(BPP), LANE_ROWS = warp_lane_rows(BPP);
    __shared__ unsigned img[WARP_LDS_DWORDS];
    __shared__ WarpTile tile;
    const int tid = threadIdx.x, f = blockIdx.z;
    const int tx0 = (int)blockIdx.x * WARP_TILE_W, ty0 = (int)blockIdx.y * TILE_H;
    if (tid == 0) {
        double M[9];
        const bool ok = warp_map(warp_frame_map(a, f), a.flags, M);
        tile.ok = ok;
        if (ok) {
            OCVAR_UNROLL
            for (int i = 0; i < 9; i++) tile.M[i] = M[i];
            const int tw = a.dw - tx0 < WARP_TILE_W ? a.dw - tx0 : WARP_TILE_W, th = a.dh - ty0 < TILE_H ? a.dh - ty0 : TILE_H;
            const WarpPlan plan = warp_tile_plan(M, tx0, ty0, tw, th, a.sw, a.sh, BPP, a.interp, a.direct ? 0 : WARP_LDS_DWORDS);
            tile.plan = plan;
            tile.recip = plan.row_dwords > 1 ? (unsigned)((0x100000000ull + (unsigned)plan.row_dwords - 1) / (unsigned)plan.row_dwords) : 0u;
        }
        if (a.status && blockIdx.x == 0 && blockIdx.y == 0) a.status[f] = ok ? 1 : 0;
    }
    __syncthreads();
    if (!tile.ok) return;      // a skipped frame: nothing of it is written
    const WarpPlan p = tile.plan;
    const uint8_t* src = a.src + (long long)f * a.src_frame_stride;
    const long long rs = a.src_row_stride;
    if (p.staged) {            // (the same for every lane of the workgroup)
        const bool src_dwords = frames_dwords(a.src, a.src_row_stride, a.src_frame_stride);
        const int row_bytes = a.sw * BPP;
        const unsigned recip = tile.recip;
        // the window's dwords, row after row, dealt to the 256 lanes in turn, WARP_STAGE_LOADS per lane in flight before the first
        // is written to LDS.  The spare dword of a row and the two behind the image are never written: the pixel loop below reads
        // them only into bytes that its shifts and masks drop.
        const int total = p.h * p.row_dwords;
        for (int base = tid; base < total; base += WARP_STAGE_LOADS * WARP_THREADS) {
            unsigned v[WARP_STAGE_LOADS];
            int at[WARP_STAGE_LOADS];
            OCVAR_UNROLL
            for (int k = 0; k < WARP_STAGE_LOADS; k++) {
                const int i = base + k * WARP_THREADS;
                v[k] = 0;
                at[k] = -1;
                if (i < total) {
                    const int r = p.row_dwords > 1 ? (int)__umulhi((unsigned)i, recip) : i, j = i - r * p.row_dwords;
                    const int b = p.b0 + 4 * j;          // the dword's first byte in the row; b < row_bytes
                    const uint8_t* row = src + (long long)(p.y0 + r) * rs;
                    at[k] = r * p.pitch + j;
                    if (src_dwords && b + 4 <= row_bytes) {
                        v[k] = *reinterpret_cast<const unsigned*>(row + b);
                    } else {
                        OCVAR_UNROLL
                        for (int e = 0; e < 4; e++)
                            if (b + e < row_bytes) v[k] |= (unsigned)row[b + e] << (8 * e);
                    }
                }
            }
            OCVAR_UNROLL
            for (int k = 0; k < WARP_STAGE_LOADS; k++)
                if (at[k] >= 0) img[at[k]] = v[k];
        }
        __syncthreads();
    }
    const int x0 = tx0 + (tid & (WARP_TILE_W / WARP_LANE_PX - 1)) * WARP_LANE_PX;
    if (x0 >= a.dw) return;
    double M[9];
    OCVAR_UNROLL
    for (int i = 0; i < 9; i++) M[i] = tile.M[i];
    const uint8_t* lds = reinterpret_cast<const uint8_t*>(img);
    const bool linear = a.interp == OCVAR_WARP_LINEAR;
    const double scale = warp_scale(a.interp);
    const int npx = a.dw - x0 < WARP_LANE_PX ? a.dw - x0 : WARP_LANE_PX;
    OCVAR_UNROLL
    for (int rr = 0; rr < LANE_ROWS; rr++) {
        const int y = ty0 + tid / (WARP_TILE_W / WARP_LANE_PX) + rr * WARP_ROW_STEP;
        if (y >= a.dh) break;
        unsigned q[BPP];
        OCVAR_UNROLL
        for (int j = 0; j < BPP; j++) q[j] = 0;
        OCVAR_UNROLL
        for (int i = 0; i < WARP_LANE_PX; i++) {
            if (x0 + i >= a.dw) continue;
            int X, Y;
            warp_source_fixed(M, x0 + i, y, scale, &X, &Y);
            const int ix = X >> 5, iy = Y >> 5;    // (inside the window they are what the core's clamp to 16 bits leaves)
            if (linear && p.staged && ix >= p.x0 && ix + 1 < p.x0 + p.w && iy >= p.y0 && iy + 1 < p.y0 + p.h) {
                int w[4];
                warp_weights(X & 31, Y & 31, w);
                const int o = ix * BPP - p.b0, s = o & 3;
                const int at = (iy - p.y0) * p.pitch + (o >> 2);
                // the two neighbouring pixels of the upper and of the lower source row, from bit 0.  d1 and d2 may be a row's
                // spare dword (never written): then s is such that none of its bytes reaches the bits read below.
                unsigned long long t[2];
                OCVAR_UNROLL
                for (int k = 0; k < 2; k++) {
                    const unsigned d0 = img[at + k * p.pitch], d1 = img[at + k * p.pitch + 1];
                    if constexpr (BPP == 1) {
                        t[k] = align_bytes(d1, d0, s);
                    } else if constexpr (BPP == 4) {
                        t[k] = (unsigned long long)d0 | ((unsigned long long)d1 << 32);
                    } else {
                        const unsigned d2 = img[at + k * p.pitch + 2];
                        t[k] = (unsigned long long)align_bytes(d1, d0, s) | ((unsigned long long)align_bytes(d2, d1, s) << 32);
                    }
                }
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) {
                    const int p00 = (int)(t[0] >> (8 * c)) & 255, p01 = (int)(t[0] >> (8 * (BPP + c))) & 255;
                    const int p10 = (int)(t[1] >> (8 * c)) & 255, p11 = (int)(t[1] >> (8 * (BPP + c))) & 255;
                    run_put(q, i * BPP + c, (p00 * w[0] + p01 * w[1] + p10 * w[2] + p11 * w[3] + 16384) >> 15);
                }
            } else {
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) {
                    const int b = warp_sample(
                        [&](int sx, int sy) -> int {
                            if (p.staged && sx >= p.x0 && sx < p.x0 + p.w && sy >= p.y0 && sy < p.y0 + p.h)
                                return lds[4 * ((sy - p.y0) * p.pitch) + sx * BPP - p.b0 + c];
                            return src[(long long)sy * rs + (long long)sx * BPP + c];
                        },
                        a.sw, a.sh, X, Y, a.interp, a.border, a.fill[c]);
                    run_put(q, i * BPP + c, b & 255);
                }
            }
        }
        uint8_t* out = a.dst + (long long)f * a.dst_frame_stride + (long long)y * a.dst_row_stride + (long long)x0 * BPP;
        run_store(q, out, ALIGNED && npx == WARP_LANE_PX, npx * BPP);
    }
}

template <int BPP>
static void launch_bpp(const WarpArgs& a, int n_frames, hipStream_t stream) {
    const dim3 grid((a.dw + WARP_TILE_W - 1) / WARP_TILE_W, (a.dh + warp_tile_h(BPP) - 1) / warp_tile_h(BPP), n_frames);
    const bool aligned = frames_dwords(a.dst, a.dst_row_stride, a.dst_frame_stride);
    if (aligned) hipLaunchKernelGGL((warp_kernel<BPP, true>), grid, dim3(WARP_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((warp_kernel<BPP, false>), grid, dim3(WARP_THREADS), 0, stream, a);
}

void launch_warp(const WarpArgs& a, int n_frames, int format, hipStream_t stream) {
    if (n_frames <= 0 || a.sw <= 0 || a.sh <= 0 || a.dw <= 0 || a.dh <= 0) return;
    switch (format_bpp(format)) {
        case 1: launch_bpp<1>(a, n_frames, stream); break;
        case 3: launch_bpp<3>(a, n_frames, stream); break;
        case 4: launch_bpp<4>(a, n_frames, stream); break;
        default: break;
    }
}

// One lane per record slot k < min(count, slots) of every frame (blockIdx: 64 slots, frame); the other slots are not written.
// A lane reads its record before it writes it, so out may be in.
__global__ __launch_bounds__(64) void warp_records_kernel(WarpRecArgs a) {
    const int k = (int)blockIdx.x * 64 + (int)threadIdx.x, f = blockIdx.y;
    int n = a.counts[f];
    n = n < a.slots ? n : a.slots;
    if (k >= n) return;
    const double* mp = (a.flags & OCVAR_WARP_ONE_MAP) ? a.maps : a.maps + 9 * (long long)f;
    double m[9];
    OCVAR_UNROLL
    for (int i = 0; i < 9; i++) m[i] = mp[i];
    MarkerRec r = a.in[(size_t)f * a.slots + k];
    warp_record(r, m, a.flags, a.cam);
    a.out[(size_t)f * a.slots + k] = r;
}

void launch_warp_records(const WarpRecArgs& a, int n_frames, hipStream_t stream) {
    if (n_frames <= 0 || a.slots <= 0) return;
    hipLaunchKernelGGL(warp_records_kernel, dim3((a.slots + 63) / 64, n_frames), dim3(64), 0, stream, a);
}

// One lane per frame: the nine doubles of its pose's plane map.
__global__ __launch_bounds__(64) void warp_board_maps_kernel(WarpBoardMapArgs a) {
    const long long f = (long long)blockIdx.x * 64 + threadIdx.x;
    if (f >= a.n_frames) return;
    const OcvarBoardPose pose = a.poses[f];
    double M[9];
    warp_board_plane_map(pose, a.K, a.rect, a.dw, a.dh, M);
    OCVAR_UNROLL
    for (int i = 0; i < 9; i++) a.maps[9 * f + i] = M[i];
}

void launch_warp_board_maps(const WarpBoardMapArgs& a, hipStream_t stream) {
    if (a.n_frames <= 0) return;
    hipLaunchKernelGGL(warp_board_maps_kernel, dim3((a.n_frames + 63) / 64), dim3(64), 0, stream, a);
}

}  // namespace ocvar
