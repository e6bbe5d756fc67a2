// order.hip -- the per-frame ordering that turns the frame pass's surviving quads into the reference's square sequence and into
// crop work for the second pass (gfx950).
//
// order_and_crops_kernel replaces cvarGetAllSquares (opencvar.cpp:564-590), the tracking loop (635-668) and
// the crop rectangle set-up of the candidate loop (676-693); dense contexts run the same tail as four scalable kernels.
#include "kernels.h"

namespace ocvar {

// Crop rectangle of square i of frame f (corners sq) and its binarise work units for the second pass (opencvar.cpp:676-693).
__device__ __forceinline__ void setup_crop(const Workspace& ws, int f, int i, const float* sq) {
    int quad[8];
    for (int k = 0; k < 8; k++) quad[k] = (int)sq[k];
    int x0, y0, cw, ch, roi_index = -1;
    crop_rect(quad, ws.W, ws.H, &x0, &y0, &cw, &ch);
    const int sw = cw & ~1, sh = ch & ~1, ns = (sw + 15) & ~15;
    if (sw >= 2 && sh >= 2) {
        const int r = atomicAdd(ws.counters + CNT_CROP_ROIS, 1);
        const long long plane = nbr_plane_bytes(ns, sh);
        const long long off = (long long)atomicAdd(ws.crop_pixels, (unsigned long long)plane);
        const int ntx = (sw + MARCH_STRIP - 1) / MARCH_STRIP, nty = (sh + MARCH_CROP_ROWS - 1) / MARCH_CROP_ROWS;
        if (r >= ws.cap_crop_rois || off + plane > ws.cap_crop_pixels) {
            atomicOr(ws.counters + CNT_ERR, ERR_CROP_OVERFLOW);
        } else {
            const int tbase = atomicAdd(ws.counters + CNT_CROP_TILES, ntx * nty);
            if (tbase + ntx * nty > ws.cap_crop_tiles) {
                atomicOr(ws.counters + CNT_ERR, ERR_TILE_OVERFLOW);
            } else {
                Roi roi;
                roi.frame = f; roi.x0 = x0; roi.y0 = y0; roi.w = cw; roi.h = ch; roi.sw = sw; roi.sh = sh; roi.ns = ns;
                roi.owner = i; roi.nbr_off = off;
                ws.rois_crop[r] = roi;
                ws.best_crop[r] = ~0ull;
                ws.crop_min_rest[r] = 0x7fffffff;
                ws.ring_crop[r] = 0;   // (ring_quads_kernel sets it where the crop's own frame border needs no walk)
                for (int t = 0; t < ntx * nty; t++) {
                    TileDesc td;
                    td.roi = r; td.x0 = t % ntx; td.y0 = (t / ntx) * MARCH_CROP_ROWS;
                    ws.tiles_crop[tbase + t] = td;
                }
                roi_index = r;
            }
        }
    }
    ws.crop_of[(size_t)f * ws.maxq + i] = roi_index;
}

__global__ __launch_bounds__(256) void order_and_crops_kernel(Workspace ws) {
    extern __shared__ int order_lds[];              // [maxq] discovery positions, then [maxq][8] ordered corners
    int* s_start = order_lds;
    float (*s_sq)[8] = reinterpret_cast<float (*)[8]>(order_lds + ws.maxq);
    __shared__ int s_n;
    const int f = blockIdx.x;
    const int tid = threadIdx.x;
    int n = ws.n_quads_frame[f];
    if (n > ws.maxq) n = ws.maxq;
    const QuadRec* q = ws.quads_frame + (size_t)f * ws.maxq;
    for (int i = tid; i < n; i += blockDim.x) s_start[i] = q[i].start;
    __syncthreads();
    // sequence order of cvarFindSquares: contours come out last-discovered first (opencvar.cpp:187-214)
    for (int i = tid; i < n; i += blockDim.x) {
        const int mine = s_start[i];
        int rank = 0;
        for (int u = 0; u < n; u++) rank += s_start[u] > mine;
        for (int k = 0; k < 8; k++) s_sq[rank][k] = (float)q[i].pt[k];
    }
    __syncthreads();
    if (tid == 0) {
        int nr = 0, nn = n;
        const int np = ws.n_prev[f];
        if (np > 0)
            nn = track_markers(ws.prev + (size_t)f * MAXM, np < MAXM ? np : MAXM, &s_sq[0][0], n, ws.reserve + (size_t)f * MAXM,
                               MAXM, &nr);   // (dense contexts: track_replay_kernel below)
        ws.n_reserve[f] = nr;
        ws.n_squares[f] = nn;
        s_n = nn;
    }
    __syncthreads();
    n = s_n;
    for (int i = tid; i < n; i += blockDim.x) {
        float* out = ws.squares + ((size_t)f * ws.maxq + i) * 8;
        for (int k = 0; k < 8; k++) out[k] = s_sq[i][k];
        setup_crop(ws, f, i, s_sq[i]);
    }
}

// ---- dense contexts (ocvar_hip_create_dense): the same per-frame tail for up to 16384 squares and 4096 markers ----------------
// order_and_crops_kernel holds a frame's squares in LDS (maxq x 9 ints), ranks them with an O(n^2) count and replays the
// tracking loop on one lane (O(markers x squares)).  Dense contexts cut it in four launches:
//   order_sort_kernel   (frame, chunk of ws.order_chunk squares: ORDER_CHUNK, or maxq rounded up to a power of two when that
//                       is smaller): the chunk's discovery positions bitonic-sorted in LDS
//   order_place_kernel  (frame, chunk): square i goes to slot "squares with a larger position" (the rank rule of
//                       order_and_crops_kernel, same slot for every input), counted by binary search in every sorted chunk
//   track_replay_kernel (frame): the corner grid and the sparse tracking replay (tail_core.h: track_markers_sparse), then the
//                       list compacted into ws.squares; a frame without previous markers only copies
//   crops_kernel        (frame, chunk): setup_crop of every square
constexpr int ORDER_THREADS = ORDER_CHUNK / 2;

__global__ __launch_bounds__(ORDER_THREADS) void order_sort_kernel(Workspace ws) {
    __shared__ int s_key[ORDER_CHUNK];
    const int CH = ws.order_chunk;   // a power of two <= ORDER_CHUNK; the block has max(64, CH / 2) threads
    const int nch = (ws.maxq + CH - 1) / CH;
    const int f = blockIdx.x / nch, c = blockIdx.x % nch;
    int n = ws.n_quads_frame[f];
    if (n > ws.maxq) n = ws.maxq;
    const int lo = c * CH, len = n - lo < CH ? n - lo : CH;
    if (len <= 0) return;
    const QuadRec* q = ws.quads_frame + (size_t)f * ws.maxq + lo;
    const int tid = threadIdx.x;
    for (int k = tid; k < CH; k += blockDim.x) s_key[k] = k < len ? q[k].start : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= CH; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < CH / 2) bitonic_step(s_key, k, j, tid);
            __syncthreads();
        }
    int* out = ws.sorted_starts + (size_t)f * ws.maxq + lo;
    for (int k = tid; k < len; k += blockDim.x) out[k] = s_key[k];
}

__global__ __launch_bounds__(256) void order_place_kernel(Workspace ws) {
    const int CH = ws.order_chunk;
    const int nch = (ws.maxq + CH - 1) / CH;
    const int f = blockIdx.x / nch, c = blockIdx.x % nch;
    int n = ws.n_quads_frame[f];
    if (n > ws.maxq) n = ws.maxq;
    const int lo = c * CH, hi = n < lo + CH ? n : lo + CH;
    const QuadRec* q = ws.quads_frame + (size_t)f * ws.maxq;
    const int* sorted = ws.sorted_starts + (size_t)f * ws.maxq;
    for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) {
        const QuadRec qi = q[i];
        int rank = 0;
        for (int b = 0; b < n; b += CH) rank += count_greater_sorted(sorted + b, n - b < CH ? n - b : CH, qi.start);
        float* out = ws.sq_tmp + ((size_t)f * ws.maxq + rank) * 8;
        for (int k = 0; k < 8; k++) out[k] = (float)qi.pt[k];
    }
}

constexpr int REPLAY_THREADS = 1024;

__global__ __launch_bounds__(REPLAY_THREADS) void track_replay_kernel(Workspace ws) {
    __shared__ int s_part[REPLAY_THREADS];
    __shared__ int s_left;
    const int f = blockIdx.x, tid = threadIdx.x;
    int n = ws.n_quads_frame[f];
    if (n > ws.maxq) n = ws.maxq;
    const int np_in = ws.n_prev[f];
    const int np = np_in < ws.maxm ? np_in : ws.maxm;
    const float* tmp = ws.sq_tmp + (size_t)f * ws.maxq * 8;
    float* sq = ws.squares + (size_t)f * ws.maxq * 8;
    if (np <= 0 || n == 0) {
        for (int e = tid; e < n * 8; e += REPLAY_THREADS) sq[e] = tmp[e];
        if (tid == 0) {
            ws.n_reserve[f] = 0;
            ws.n_squares[f] = n;
        }
        return;
    }
    const int gw = ws.track_gw, gh = ws.track_gh, nc = gw * gh;
    int* cells = ws.trk_cells + (size_t)f * (nc + 1);
    int* fill = ws.trk_fill + (size_t)f * nc;
    int* items = ws.trk_items + (size_t)f * 4 * ws.maxq;
    int* next = ws.trk_next + (size_t)f * (ws.maxq + 1);
    // the corner grid (tail_core.h: track_grid_build, in parallel): counts, exclusive scan, fill
    for (int c = tid; c < nc; c += REPLAY_THREADS) fill[c] = 0;
    __syncthreads();
    for (int j = tid; j < 4 * n; j += REPLAY_THREADS)
        atomicAdd(fill + track_cell(tmp[2 * j + 1], gh) * gw + track_cell(tmp[2 * j], gw), 1);
    __syncthreads();
    const int per = (nc + REPLAY_THREADS - 1) / REPLAY_THREADS, c0 = tid * per, c1 = c0 + per < nc ? c0 + per : nc;
    int sum = 0;
    // (the counts were made by atomics at L2: read them past the L1)
    for (int c = c0; c < c1; c++) sum += __hip_atomic_load(fill + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < REPLAY_THREADS; d <<= 1) {   // inclusive scan of the threads' sums
        const int v = tid >= d ? s_part[tid - d] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int run = s_part[tid] - sum;
    for (int c = c0; c < c1; c++) {
        const int k = __hip_atomic_load(fill + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cells[c] = run;
        fill[c] = run;
        run += k;
    }
    if (tid == 0) cells[nc] = 4 * n;
    __syncthreads();
    for (int j = tid; j < 4 * n; j += REPLAY_THREADS)
        items[atomicAdd(fill + track_cell(tmp[2 * j + 1], gh) * gw + track_cell(tmp[2 * j], gw), 1)] = j >> 2;
    __syncthreads();
    // the replay itself is sequential (each marker sees the erasures of the ones before it) but sparse
    if (tid == 0) {
        int nr = 0;
        s_left = track_markers_sparse(ws.prev + (size_t)f * ws.maxm, np, tmp, n, cells, items, gw, gh, next,
                                      ws.reserve + (size_t)f * ws.maxm, ws.maxm, &nr);
        ws.n_reserve[f] = nr;
        ws.n_squares[f] = s_left;
    }
    __syncthreads();
    // the squares still in the list, in list order (block-wide prefix count over chunks of REPLAY_THREADS)
    int base = 0;
    for (int b = 0; b < n; b += REPLAY_THREADS) {
        const int i = b + tid;
        const int keep = i < n && next[i] == i;
        s_part[tid] = keep;
        __syncthreads();
        for (int d = 1; d < REPLAY_THREADS; d <<= 1) {
            const int v = tid >= d ? s_part[tid - d] : 0;
            __syncthreads();
            s_part[tid] += v;
            __syncthreads();
        }
        if (keep) {
            const int o = base + s_part[tid] - 1;
            for (int k = 0; k < 8; k++) sq[(size_t)o * 8 + k] = tmp[(size_t)i * 8 + k];
        }
        base += s_part[REPLAY_THREADS - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void crops_kernel(Workspace ws) {
    const int CH = ws.order_chunk;
    const int nch = (ws.maxq + CH - 1) / CH;
    const int f = blockIdx.x / nch, c = blockIdx.x % nch;
    int n = ws.n_squares[f];
    if (n > ws.maxq) n = ws.maxq;
    const int hi = n < (c + 1) * CH ? n : (c + 1) * CH;
    for (int i = c * CH + (int)threadIdx.x; i < hi; i += blockDim.x) setup_crop(ws, f, i, ws.squares + ((size_t)f * ws.maxq + i) * 8);
}

void launch_order_and_crops(const Workspace& ws, hipStream_t stream) {
    if (ws.n_frames > 0 && ws.dense) {
        const int grid = ws.n_frames * ((ws.maxq + ws.order_chunk - 1) / ws.order_chunk);
        hipLaunchKernelGGL(order_sort_kernel, dim3(grid), dim3(ws.order_chunk / 2 > 64 ? ws.order_chunk / 2 : 64), 0, stream, ws);
        hipLaunchKernelGGL(order_place_kernel, dim3(grid), dim3(256), 0, stream, ws);
        hipLaunchKernelGGL(track_replay_kernel, dim3(ws.n_frames), dim3(REPLAY_THREADS), 0, stream, ws);
        hipLaunchKernelGGL(crops_kernel, dim3(grid), dim3(256), 0, stream, ws);
        return;
    }
    if (ws.n_frames > 0) hipLaunchKernelGGL(order_and_crops_kernel, dim3(ws.n_frames), dim3(ws.maxq <= 256 ? 64 : 256) /* one wave: starts wherever a SIMD has room */, (size_t)ws.maxq * 9 * sizeof(int), stream, ws);
}

}  // namespace ocvar
