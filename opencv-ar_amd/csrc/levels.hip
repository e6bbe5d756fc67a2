// levels.hip -- opt-in stretching of the grey levels of device-resident frames, per frame or per tile with blended maps
// (ocvar_hip_levels).  The definition is levels_core.h's; its host build (tests/emul/levels_emul.cpp) gives these kernels' bytes.
// Three kernels on one stream, one round for at most LEVELS_WS_FRAMES frames; the arguments travel by value.
//
//   histogram  one workgroup of 4 waves per (row slab of LEVELS_SLAB_ROWS rows, tile, frame); tiles of fewer slabs leave their
//              surplus workgroups at once.  A wave takes every fourth row of the slab, a lane runs of 4 pixels that start at
//              multiples of 4 in the FRAME's x, so that with ALIGNED (source address, row stride and frame stride multiples of 4) a
//              run inside the tile is BPP whole dwords; the runs a tile edge cuts, and everything when something is unaligned, are
//              read byte by byte.  Grey is taken in registers.  Counts go to an LDS histogram with ds_add_u32 and from there, the
//              bins that are not zero only, onto the frame's tile histogram in the workspace with global 32-bit integer atomics:
//              integer adds commute, the result does not depend on scheduling.
//              Contention: on a constant frame every lane hits one bin.  Two measures.  A lane first combines the equal values
//              among its own 4 pixels (one add of 4 instead of four adds of 1 on a flat run).  And the workgroup keeps
//              LEVELS_COPIES = 8 histograms, lane l adding to copy l & 7, interleaved bin-major (bin v of copy k is word 8 v + k):
//              the 8 copies of a bin lie in 8 different banks, so the 32 lanes of a group that all hold one value make 8
//              addresses of 4 lanes each instead of one address of 32.  8 KiB of LDS per workgroup.
//   LUT        one wave per (tile, frame): a lane loads 4 consecutive bins as one 16-byte load and stores 16 zero bytes in their
//              place -- THE HISTOGRAM IS LEFT ZEROED FOR THE NEXT USE; the workspace is cleared once, when it is allocated --,
//              prefix sums over the wave with 6 shuffles, lo and hi by a wave minimum and maximum, the gain cap, and its 4 bytes of
//              the LUT as one dword.
//   apply      one workgroup of 4 waves per rectangle of at most LEVELS_SEG_W x LEVELS_SEG_H pixels that lies within one cell of
//              the tile-centre lattice (levels_core.h: levels_segment): all its pixels blend the same at most four LUTs, which are
//              staged in LDS interleaved -- word g holds lut[j0][i0][g], lut[j0][i1][g], lut[j1][i0][g], lut[j1][i1][g] in its four
//              bytes, 1 KiB -- so that a pixel's four values are one ds_read_b32 at a data-dependent address.  The x weights are
//              computed once per lane and run (they do not depend on the row), the y weights once per workgroup into LDS.  Runs of 4
//              pixels as in the histogram kernel; with ALIGNED (both sides) a full run is stored as one dword, everything else byte
//              by byte: no byte outside the destination's pixels is written, and the source is never written.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int LEVELS_THREADS = 256;
constexpr int LEVELS_COPIES = 8;

// The greys of the 4 pixels of a full run at p.
template <int BPP, bool ALIGNED>
OCVAR_D void levels_run_grey(const uint8_t* p, int fmt, int (&g)[4]) {
    unsigned w[BPP];
    run_load(w, p, ALIGNED, 4 * BPP);
    OCVAR_UNROLL
    for (int i = 0; i < 4; i++) {
        if constexpr (BPP == 1) g[i] = run_byte(w, i);
        else g[i] = levels_grey(run_byte(w, i * BPP), run_byte(w, i * BPP + 1), run_byte(w, i * BPP + 2), fmt);
    }
}

template <int BPP>
OCVAR_D int levels_px_grey(const uint8_t* p, int fmt) {
    if constexpr (BPP == 1) return p[0];
    else return levels_grey(p[0], p[1], p[2], fmt);
}

template <int BPP, bool ALIGNED>
__global__ __launch_bounds__(LEVELS_THREADS) void levels_hist_kernel(LevelsArgs a, int fmt) {
    __shared__ unsigned bins[256 * LEVELS_COPIES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.y, tj = tile / a.p.tiles_x, ti = tile - tj * a.p.tiles_x;
    const int x0 = levels_edge(ti, a.w, a.p.tiles_x), x1 = levels_edge(ti + 1, a.w, a.p.tiles_x);
    const int ye = levels_edge(tj + 1, a.h, a.p.tiles_y);
    const int y0 = levels_edge(tj, a.h, a.p.tiles_y) + (int)blockIdx.x * LEVELS_SLAB_ROWS;
    if (y0 >= ye) return;      // (the whole workgroup: this tile has fewer slabs than the tallest one)
    const int y1 = ye - y0 < LEVELS_SLAB_ROWS ? ye : y0 + LEVELS_SLAB_ROWS;
    OCVAR_UNROLL
    for (int i = tid; i < 256 * LEVELS_COPIES; i += LEVELS_THREADS) bins[i] = 0;
    __syncthreads();
    const uint8_t* src = a.src + (long long)blockIdx.z * a.src_frame_stride;
    unsigned* mine = bins + (lane & (LEVELS_COPIES - 1));
    const int q1 = (x1 + 3) >> 2;
    for (int y = y0 + wave; y < y1; y += LEVELS_THREADS / 64) {
        const uint8_t* row = src + (long long)y * a.src_row_stride;
        for (int q = (x0 >> 2) + lane; q < q1; q += 64) {
            const int xa = 4 * q;
            if (xa >= x0 && xa + 4 <= x1) {
                int g[4];
                levels_run_grey<BPP, ALIGNED>(row + (long long)xa * BPP, fmt, g);
                // equal values among the lane's four are added once
                atomicAdd(&mine[g[0] * LEVELS_COPIES], 1u + (g[1] == g[0]) + (g[2] == g[0]) + (g[3] == g[0]));
                if (g[1] != g[0]) atomicAdd(&mine[g[1] * LEVELS_COPIES], 1u + (g[2] == g[1]) + (g[3] == g[1]));
                if (g[2] != g[0] && g[2] != g[1]) atomicAdd(&mine[g[2] * LEVELS_COPIES], 1u + (g[3] == g[2]));
                if (g[3] != g[0] && g[3] != g[1] && g[3] != g[2]) atomicAdd(&mine[g[3] * LEVELS_COPIES], 1u);
            } else {
                for (int x = xa < x0 ? x0 : xa; x < xa + 4 && x < x1; x++)
                    atomicAdd(&mine[levels_px_grey<BPP>(row + (long long)x * BPP, fmt) * LEVELS_COPIES], 1u);
            }
        }
    }
    __syncthreads();
    unsigned s = 0;
    OCVAR_UNROLL
    for (int k = 0; k < LEVELS_COPIES; k++) s += bins[tid * LEVELS_COPIES + k];
    if (s) atomicAdd(&a.hist[((size_t)blockIdx.z * LEVELS_MAX_TILES + tile) * 256 + tid], s);
}

__global__ __launch_bounds__(64) void levels_lut_kernel(LevelsArgs a) {
    const int lane = threadIdx.x;
    const size_t slot = (size_t)blockIdx.y * LEVELS_MAX_TILES + blockIdx.x;
    uint4* h = reinterpret_cast<uint4*>(a.hist + slot * 256) + lane;
    const uint4 c = *h;
    *h = make_uint4(0u, 0u, 0u, 0u);
    const unsigned cnt[4] = {c.x, c.y, c.z, c.w};
    unsigned cum[4];      // #{g <= 4 lane + k}
    cum[0] = cnt[0], cum[1] = cum[0] + cnt[1], cum[2] = cum[1] + cnt[2], cum[3] = cum[2] + cnt[3];
    unsigned inc = cum[3];
    OCVAR_UNROLL
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    const unsigned before = inc - cum[3], n = __shfl(inc, 63, 64);
    const unsigned long long k_lo = levels_clip_count(n, a.p.low_ppm), k_hi = levels_clip_count(n, a.p.high_ppm);
    int lo = 256, hi = -1;
    OCVAR_UNROLL
    for (int k = 3; k >= 0; k--)
        if ((unsigned long long)(before + cum[k]) > k_lo) lo = 4 * lane + k;
    OCVAR_UNROLL
    for (int k = 0; k < 4; k++)      // #{g >= v} = n - #{g <= v - 1}
        if ((unsigned long long)(n - (before + cum[k] - cnt[k])) > k_hi) hi = 4 * lane + k;
    OCVAR_UNROLL
    for (int d = 1; d < 64; d <<= 1) {
        const int l2 = __shfl_xor(lo, d, 64), h2 = __shfl_xor(hi, d, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    lo = lo > 255 ? 255 : lo;     // (n >= 1 and k < n: both exist)
    hi = hi < 0 ? 0 : hi;
    levels_cap(&lo, &hi, a.p.max_gain_q8);
    unsigned out = 0;
    OCVAR_UNROLL
    for (int k = 0; k < 4; k++) out |= (unsigned)levels_lut_value(4 * lane + k, lo, hi) << (8 * k);
    reinterpret_cast<unsigned*>(a.luts + slot * 256)[lane] = out;
}

template <int BPP, bool ALIGNED>
__global__ __launch_bounds__(LEVELS_THREADS) void levels_apply_kernel(LevelsArgs a, int fmt) {
    __shared__ unsigned lut4[256];
    __shared__ int wys[LEVELS_SEG_H];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = a.p.tiles_x, ty = a.p.tiles_y;
    int ci, sx, nx, cj, sy, ny;
    levels_segment(blockIdx.x, a.w, tx, LEVELS_SEG_W, &ci, &sx, &nx);
    levels_segment(blockIdx.y, a.h, ty, LEVELS_SEG_H, &cj, &sy, &ny);
    const int i1 = ci + 1 < tx ? ci + 1 : tx - 1, j1 = cj + 1 < ty ? cj + 1 : ty - 1;
    int ax, bx, ay, by;
    levels_cell_centres(ci, a.w, tx, &ax, &bx);
    levels_cell_centres(cj, a.h, ty, &ay, &by);
    {
        const uint8_t* L = a.luts + (size_t)blockIdx.z * LEVELS_MAX_TILES * 256 + tid;
        lut4[tid] = (unsigned)L[(cj * tx + ci) * 256] | ((unsigned)L[(cj * tx + i1) * 256] << 8) | ((unsigned)L[(j1 * tx + ci) * 256] << 16) |
                    ((unsigned)L[(j1 * tx + i1) * 256] << 24);
        if (tid < ny) wys[tid] = levels_weight(sy + tid, ay, by);
    }
    __syncthreads();
    const uint8_t* src = a.src + (long long)blockIdx.z * a.src_frame_stride;
    uint8_t* dst = a.dst + (long long)blockIdx.z * a.dst_frame_stride;
    const int x1 = sx + nx;
    for (int q = (sx >> 2) + lane; 4 * q < x1; q += 64) {
        const int xa = 4 * q;
        const bool full = xa >= sx && xa + 4 <= x1;
        int wx[4];
        OCVAR_UNROLL
        for (int i = 0; i < 4; i++) wx[i] = levels_weight(xa + i, ax, bx);
        for (int r = wave; r < ny; r += LEVELS_THREADS / 64) {
            const int wy = wys[r];
            const uint8_t* row = src + (long long)(sy + r) * a.src_row_stride;
            uint8_t* out = dst + (long long)(sy + r) * a.dst_row_stride;
            if (full) {
                int g[4];
                levels_run_grey<BPP, ALIGNED>(row + (long long)xa * BPP, fmt, g);
                unsigned o[1] = {0};
                OCVAR_UNROLL
                for (int i = 0; i < 4; i++) {
                    const unsigned t = lut4[g[i]];
                    run_put(o, i, levels_mix((int)(t & 255u), (int)((t >> 8) & 255u), (int)((t >> 16) & 255u), (int)(t >> 24), wx[i], wy));
                }
                run_store(o, out + xa, ALIGNED, 4);
            } else {
                OCVAR_UNROLL
                for (int i = 0; i < 4; i++) {
                    const int x = xa + i;
                    if (x >= sx && x < x1) {
                        const unsigned t = lut4[levels_px_grey<BPP>(row + (long long)x * BPP, fmt)];
                        out[x] = (uint8_t)levels_mix((int)(t & 255u), (int)((t >> 8) & 255u), (int)((t >> 16) & 255u), (int)(t >> 24), wx[i], wy);
                    }
                }
            }
        }
    }
}

template <int BPP>
static void launch_bpp(const LevelsArgs& a, int n_frames, int format, hipStream_t stream) {
    const bool src_dwords = frames_dwords(a.src, a.src_row_stride, a.src_frame_stride), dst_dwords = frames_dwords(a.dst, a.dst_row_stride, a.dst_frame_stride);
    const int tiles = a.p.tiles_x * a.p.tiles_y;
    const int tallest = (a.h + a.p.tiles_y - 1) / a.p.tiles_y;
    const dim3 hgrid((tallest + LEVELS_SLAB_ROWS - 1) / LEVELS_SLAB_ROWS, tiles, n_frames);
    if (src_dwords) hipLaunchKernelGGL((levels_hist_kernel<BPP, true>), hgrid, dim3(LEVELS_THREADS), 0, stream, a, format);
    else hipLaunchKernelGGL((levels_hist_kernel<BPP, false>), hgrid, dim3(LEVELS_THREADS), 0, stream, a, format);
    hipLaunchKernelGGL(levels_lut_kernel, dim3(tiles, n_frames), dim3(64), 0, stream, a);
    const dim3 agrid(levels_segments(a.w, a.p.tiles_x, LEVELS_SEG_W), levels_segments(a.h, a.p.tiles_y, LEVELS_SEG_H), n_frames);
    if (src_dwords && dst_dwords) hipLaunchKernelGGL((levels_apply_kernel<BPP, true>), agrid, dim3(LEVELS_THREADS), 0, stream, a, format);
    else hipLaunchKernelGGL((levels_apply_kernel<BPP, false>), agrid, dim3(LEVELS_THREADS), 0, stream, a, format);
}

void launch_levels(const LevelsArgs& a, int n_frames, int format, hipStream_t stream) {
    if (n_frames <= 0 || n_frames > LEVELS_WS_FRAMES || a.w <= 0 || a.h <= 0 || levels_params_bad(a.p, a.w, a.h)) return;
    switch (format_bpp(format)) {
        case 1: launch_bpp<1>(a, n_frames, format, stream); break;
        case 3: launch_bpp<3>(a, n_frames, format, stream); break;
        case 4: launch_bpp<4>(a, n_frames, format, stream); break;
        default: break;
    }
}

}  // namespace ocvar
