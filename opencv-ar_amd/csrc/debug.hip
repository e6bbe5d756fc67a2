// debug.hip -- the ocvar_hip_debug_* entry points of include/ocvar_hip.h: intermediate results of the last batch, copied out of
// the workspace for the tests and tools, and the calibration load of the traffic counters.
#include "context.h"
#include <cstring>

using namespace ocvar;

extern "C" int ocvar_hip_debug_gray(OcvarHip* c, int frame, uint8_t* h) {
    if (!c || !h || frame < 0 || frame >= c->ws.n_frames) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const int W = c->ws.W, H = c->ws.H, pitch = gray_pitch(W);
    const size_t plane = (size_t)gray_plane_bytes(W, H);
    std::vector<uint8_t> g(plane);
    HIP_TRY(c, hipMemcpy(g.data(), c->ws.gray + frame * plane, plane, hipMemcpyDeviceToHost));
    for (int y = 0; y < H; y++)   // out of the panels, into plain rows
        for (int x = 0; x < W; x++) h[(size_t)y * W + x] = g[(size_t)y * pitch + gray_col(x)];
    return OCVAR_OK;
}

// The bit plane of a frame of the last batch, expanded to a byte per pixel: the binary image itself (0 / 255; the 1-px frame is
// zero as cvFindContours makes it), or each pixel's 8-neighbour mask.
static int plane_to_host(OcvarHip* c, int frame, uint8_t* h, bool masks) {
    if (!c || !h || frame < 0 || frame >= c->ws.n_frames) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const int sw = c->ws.sw, sh = c->ws.sh, ns = c->ws.ns;
    const size_t bytes = (size_t)nbr_plane_bytes(ns, sh);
    std::vector<uint8_t> nbr(bytes);
    HIP_TRY(c, hipMemcpy(nbr.data(), c->ws.nbr_frame + (size_t)frame * bytes, bytes, hipMemcpyDeviceToHost));
    for (int y = 0; y < sh; y++)
        for (int x = 0; x < sw; x++)
            h[(size_t)y * sw + x] = masks ? (uint8_t)nbr_of(nbr.data(), x, y, ns) : (nbr_bit(nbr.data(), x, y, ns) ? 255 : 0);
    return OCVAR_OK;
}

extern "C" int ocvar_hip_debug_binary(OcvarHip* c, int frame, uint8_t* h) { return plane_to_host(c, frame, h, false); }
extern "C" int ocvar_hip_debug_masks(OcvarHip* c, int frame, uint8_t* h) { return plane_to_host(c, frame, h, true); }

int ocvar::quads_to_host(OcvarHip* c, int frame, int lim, int* quads, int* n_quads) {
    int n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->ws.n_squares + frame, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float> sq((size_t)(lim > 0 ? lim : 0) * 8);
    if (!sq.empty())
        HIP_TRY(c, hipMemcpy(sq.data(), c->ws.squares + (size_t)frame * c->ws.maxq * 8, sq.size() * sizeof(float), hipMemcpyDeviceToHost));
    *n_quads = n;
    for (int i = 0; i < n && i < lim; i++)
        for (int k = 0; k < 8; k++) quads[8 * i + k] = (int)sq[8 * (size_t)i + k];
    return OCVAR_OK;
}

extern "C" int ocvar_hip_debug_frame_quads(OcvarHip* c, int frame, int* quads, int* n_quads) {
    if (!c || !quads || !n_quads || frame < 0 || frame >= c->ws.n_frames) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    // `quads` holds OCVAR_MAX_QUADS quads (the documented size); a context made for fewer or more squares per frame
    // (ocvar_hip_create_ex) reports what both hold
    return quads_to_host(c, frame, c->ws.maxq < OCVAR_MAX_QUADS ? c->ws.maxq : OCVAR_MAX_QUADS, quads, n_quads);
}

// The crop pass of the last collected batch.  Its ROI records and bit planes stay in the workspace until the next enqueue;
// nothing is launched here.  The ROI count comes from the batch's own counter copy (collect has waited for it).
static int crop_count(const OcvarHip* c) {
    if (!c || c->pending || !c->crops_ran || c->ws.n_frames < 1 || !c->h_counters.p) return -1;
    if (c->h_counters[CNT_ERR] & (ERR_CROP_OVERFLOW | ERR_TILE_OVERFLOW)) return -1;   // (ROIs past a pool's end were never written)
    const int n = c->h_counters[CNT_CROP_ROIS];
    return n < 0 ? -1 : (n < c->ws.cap_crop_rois ? n : c->ws.cap_crop_rois);
}

extern "C" int ocvar_hip_debug_crop_rois(OcvarHip* c, OcvarCropRoi* rois, int max_rois, int* n_rois) {
    const int n = crop_count(c);
    if (n < 0 || !n_rois || max_rois < 0 || (max_rois > 0 && !rois)) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const int k = n < max_rois ? n : max_rois;
    std::vector<Roi> r((size_t)(k > 0 ? k : 1));
    if (k > 0) HIP_TRY(c, hipMemcpy(r.data(), c->ws.rois_crop, (size_t)k * sizeof(Roi), hipMemcpyDeviceToHost));
    for (int i = 0; i < k; i++) {
        OcvarCropRoi& o = rois[i];
        o.index = i; o.frame = r[i].frame; o.owner = r[i].owner;
        o.x0 = r[i].x0; o.y0 = r[i].y0; o.w = r[i].w; o.h = r[i].h;
    }
    *n_rois = n;
    return OCVAR_OK;
}

// One crop's bit plane expanded to a byte per pixel, (w & ~1) x (h & ~1), as plane_to_host does for a frame.
extern "C" int ocvar_hip_debug_crop_plane(OcvarHip* c, int roi, int masks, uint8_t* h) {
    const int n = crop_count(c);
    if (n < 0 || !h || roi < 0 || roi >= n) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    Roi r;
    HIP_TRY(c, hipMemcpy(&r, c->ws.rois_crop + roi, sizeof(Roi), hipMemcpyDeviceToHost));
    const long long bytes = r.ns > 0 && r.sh > 0 ? nbr_plane_bytes(r.ns, r.sh) : 0;
    if (r.sw < 2 || r.sh < 2 || r.sw > r.ns || (r.ns & 15) || r.nbr_off < 0 || r.nbr_off + bytes > c->ws.cap_crop_pixels) {
        c->err = "ocvar_hip_debug_crop_plane: the ROI record does not describe a plane of the crop pool";
        return OCVAR_E_ARG;
    }
    std::vector<uint8_t> nbr((size_t)bytes);
    HIP_TRY(c, hipMemcpy(nbr.data(), c->ws.nbr_crop + r.nbr_off, (size_t)bytes, hipMemcpyDeviceToHost));
    for (int y = 0; y < r.sh; y++)
        for (int x = 0; x < r.sw; x++)
            h[(size_t)y * r.sw + x] = masks ? (uint8_t)nbr_of(nbr.data(), x, y, r.ns) : (nbr_bit(nbr.data(), x, y, r.ns) ? 255 : 0);
    return OCVAR_OK;
}

// The start list of the last collected batch (binarise.hip::march_unit stages y * ns + x with the ROI's plane stride ns), with
// the positions taken apart.  The followers only read the lists, so they stay as the binarise kernels left them.
extern "C" int ocvar_hip_debug_starts(OcvarHip* c, int crop_pass, OcvarStart* starts, int max_starts, int* n_starts) {
    if (!c || c->pending || !n_starts || max_starts < 0 || (max_starts > 0 && !starts) || c->ws.n_frames < 1 || !c->h_counters.p) return OCVAR_E_ARG;
    const int n_rois = crop_pass ? crop_count(c) : c->ws.n_frames;
    if (n_rois < 0) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const int cap = crop_pass ? c->ws.cap_crop_cands : c->ws.cap_frame_cands;
    int n = c->h_counters[crop_pass ? CNT_CROP_CANDS : CNT_FRAME_CANDS];
    n = n < 0 ? 0 : n < cap ? n : cap;
    const int k = n < max_starts ? n : max_starts;
    std::vector<StartCand> sc((size_t)(k > 0 ? k : 1));
    if (k > 0) HIP_TRY(c, hipMemcpy(sc.data(), crop_pass ? c->ws.cands_crop : c->ws.cands_frame, (size_t)k * sizeof(StartCand), hipMemcpyDeviceToHost));
    std::vector<Roi> rois((size_t)(crop_pass && n_rois > 0 ? n_rois : 1));
    if (crop_pass && n_rois > 0) HIP_TRY(c, hipMemcpy(rois.data(), c->ws.rois_crop, (size_t)n_rois * sizeof(Roi), hipMemcpyDeviceToHost));
    for (int i = 0; i < k; i++) {
        const StartCand& s = sc[i];
        const int ns = crop_pass ? (s.roi >= 0 && s.roi < n_rois ? rois[s.roi].ns : 0) : c->ws.ns;
        if (s.roi < 0 || s.roi >= n_rois || ns <= 0 || s.pos < 0) {
            c->err = "ocvar_hip_debug_starts: a record of the start list does not belong to the batch";
            return OCVAR_E_ARG;
        }
        starts[i].roi = s.roi;
        starts[i].x = s.pos % ns;
        starts[i].y = s.pos / ns;
        starts[i].is_hole = s.is_hole;
    }
    *n_starts = n;
    return OCVAR_OK;
}

// The ring verdicts of the last collected batch (follow.hip::ring_quads_kernel: 1 where the ROI's own frame border is the rectangle
// that needs no walk), one int per frame or per crop ROI.  Batches of at most 8 frames run no ring kernel: api.hip and order.hip
// have cleared the flags.
extern "C" int ocvar_hip_debug_rings(OcvarHip* c, int crop_pass, int* flags, int max_flags, int* n_flags) {
    if (!c || c->pending || !n_flags || max_flags < 0 || (max_flags > 0 && !flags) || c->ws.n_frames < 1 || !c->h_counters.p) return OCVAR_E_ARG;
    const int n = crop_pass ? crop_count(c) : c->ws.n_frames;
    if (n < 0) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const int k = n < max_flags ? n : max_flags;
    if (k > 0) HIP_TRY(c, hipMemcpy(flags, crop_pass ? c->ws.ring_crop : c->ws.ring_frame, (size_t)k * sizeof(int), hipMemcpyDeviceToHost));
    *n_flags = n;
    return OCVAR_OK;
}

extern "C" int ocvar_hip_debug_candidates(OcvarHip* c, int frame, OcvarCandidate* cands, int max_cands, int* n_cands) {
    if (!c || !cands || !n_cands || frame < 0 || frame >= c->ws.n_frames) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int nsq = 0;
    HIP_TRY(c, hipMemcpy(&nsq, c->ws.n_squares + frame, sizeof(int), hipMemcpyDeviceToHost));
    if (nsq > c->ws.maxq) nsq = c->ws.maxq;
    // the compact records of the frame's squares, expanded to the reference's list: K candidates per square with a crop quad,
    // in template order, the orient 2/4 rotations accumulating over the square's templates
    const Workspace& w = c->ws;
    const Library& L = c->lib;
    const size_t first = (size_t)frame * w.maxq;
    std::vector<SquareRec> recs(nsq > 0 ? nsq : 1);
    std::vector<long long> codes((size_t)(nsq > 0 ? nsq : 1) * w.n_sizes);
    std::vector<int> match((size_t)(nsq > 0 ? nsq : 1) * w.max_match);
    if (nsq > 0) {
        HIP_TRY(c, hipMemcpy(recs.data(), w.sq_recs + first, nsq * sizeof(SquareRec), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(codes.data(), w.sq_codes + first * w.n_sizes, codes.size() * sizeof(long long), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(match.data(), w.sq_match + first * w.max_match, match.size() * sizeof(int), hipMemcpyDeviceToHost));
    }
    std::vector<int> orient_of(L.n_groups(), 0);
    long long n = 0;
    for (int i = 0; i < nsq; i++) {
        const SquareRec& r = recs[i];
        if (r.n_match < 0) continue;
        if (n >= max_cands) {   // (only the count is still wanted)
            n += w.n_templates;
            continue;
        }
        const int* m = match.data() + (size_t)i * w.max_match;
        for (int k = 0; k < r.n_match; k++) orient_of[match_group(m[k])] = match_orient_of(m[k]);
        int sh = 0;
        for (int j = 0; j < w.n_templates; j++, n++) {
            const int orient = orient_of[L.group_of[j]];
            sh = (sh + orient_shift(orient)) & 3;
            if (n >= max_cands) continue;
            OcvarCandidate& o = cands[n];
            o.markerId = i;
            o.templateId = j;
            o.orient = orient;
            o.valid = 1;
            o.bit = codes[(size_t)i * w.n_sizes + L.size_of[j]];
            shift_square(r.square, sh, o.square);
            std::memcpy(o.patPoint, r.patPoint, sizeof o.patPoint);
        }
        for (int k = 0; k < r.n_match; k++) orient_of[match_group(m[k])] = 0;
    }
    *n_cands = n > 0x7fffffff ? 0x7fffffff : (int)n;
    return OCVAR_OK;
}

// Calibration load for rocprofv3's FETCH_SIZE / WRITE_SIZE counters (MI355X_MICROARCH.md, HBM section: the
// counters are only calibrated for 16-byte-per-lane streams): copies `bytes` with the access widths the binarise kernel
// uses (one dword per lane, coalesced), so a profile of this launch gives bytes-per-counter-unit for that pattern.
__global__ void calib_copy_dword_kernel(const unsigned* src, unsigned* dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i] + 1u;
}

extern "C" int ocvar_hip_debug_calibrate(OcvarHip* c, size_t bytes) {
    if (!c || bytes < 1024) return OCVAR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned *a = nullptr, *b = nullptr;
    HIP_TRY(c, hipMalloc((void**)&a, bytes));
    HIP_TRY(c, hipMalloc((void**)&b, bytes));
    HIP_TRY(c, hipMemset(a, 1, bytes));
    hipLaunchKernelGGL(calib_copy_dword_kernel, dim3(4096), dim3(256), 0, c->stream.s, a, b, bytes / 4);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    (void)hipFree(a);
    (void)hipFree(b);
    return OCVAR_OK;
}
