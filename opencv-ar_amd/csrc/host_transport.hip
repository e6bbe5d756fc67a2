// host_transport.hip -- the entry points of include/ocvar_hip.h that take frames in host memory: staging, the pipelined
// transfers of ocvar_hip_detect_host, and ocvar_hip_find_squares.
#include "context.h"
#include <algorithm>
#include <cstring>
#include <thread>

using namespace ocvar;

// one batch of frames through the first page-locked staging buffer into the device staging, on the context's stream
static int stage_frames(OcvarHip* c, const uint8_t* h, int height, int row_stride, size_t frame_stride, int n_frames) {
    const size_t bytes = (size_t)(n_frames - 1) * frame_stride + (size_t)height * row_stride;
    HIP_TRY(c, c->d_frames.reserve(bytes));
    for (auto& b : c->h_stage) HIP_TRY(c, b.reserve(bytes));
    std::memcpy(c->h_stage[0], h, bytes);
    HIP_TRY(c, hipMemcpyAsync(c->d_frames, c->h_stage[0], bytes, hipMemcpyHostToDevice, c->stream));
    return OCVAR_OK;
}

// A host-to-host copy of a sub-batch (hundreds of megabytes at 1080p) by a few threads: one core copies ~10 GB/s, the PCIe
// link behind it takes 46.
static void host_copy(uint8_t* dst, const uint8_t* src, size_t n) {
    constexpr size_t PIECE = (size_t)4 << 20;
    unsigned nt = (unsigned)std::min<size_t>(8, n / PIECE);
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && nt > hw) nt = hw;
    if (nt < 2) {
        std::memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t per = ((n / nt) + 63) & ~(size_t)63;
    for (unsigned t = 1; t < nt; t++) {
        const size_t off = per * t, len = off >= n ? 0 : std::min(per, n - off);
        if (!len) continue;
        try {
            th.emplace_back([=] { std::memcpy(dst + off, src + off, len); });
        } catch (...) {   // no thread to be had: this piece is copied here (nothing is thrown across the C ABI)
            std::memcpy(dst + off, src + off, len);
        }
    }
    std::memcpy(dst, src, std::min(per, n));
    for (auto& t : th) t.join();
}

// is [p, p + bytes) host memory the CALLER has page-locked (hipHostMalloc / hipHostRegister on their side)?
static bool caller_pinned(const uint8_t* p, size_t bytes) {
    hipPointerAttribute_t a{}, b{};
    const bool ok = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost &&
                    hipPointerGetAttributes(&b, p + bytes - 1) == hipSuccess && b.type == hipMemoryTypeHost;
    (void)hipGetLastError();   // "not a HIP pointer" is the ordinary answer for pageable memory
    return ok;
}

// Frames in host memory (the reference's caller hands a host IplImage, samples/ARTest.cpp:44-57).
// The call is cut into sub-batches; while the kernels of sub-batch k run, sub-batch k+1 is copied into one of the context's two
// page-locked staging buffers (by a few host threads) and from there to the device by the copy engine, and the in-place grey of
// sub-batch k-1 (opencvar.cpp:624-627) travels back the same way on a third stream.  The library NEVER page-locks the caller's
// memory (no hipHostRegister / hipHostUnregister: round 2's version did that, and a small heap-resident batch -- which shares
// its first and last page with whatever malloc put next to it -- ended in a GPU memory fault on a host address; DESIGN.md
// section 9 lists what that range shared pages with).  A caller that wants the copies straight from its own buffer
// page-locks it itself (hipHostMalloc, or hipHostRegister for as long as it likes): such a buffer is recognised
// (hipPointerGetAttributes) and used in place.  The two page-locked staging buffers are the library's own: the only host memory
// of a frame transfer the copy engines ever see, unless the caller's buffer is page-locked by the caller.
constexpr int HOST_SUB_BATCH = 64;

extern "C" int ocvar_hip_detect_host(OcvarHip* c, uint8_t* h_bgr, int width, int height, int row_stride, size_t frame_stride,
                                     int n_frames, int grey_in_place, const OcvarMarker* prev, const int* prev_counts,
                                     OcvarMarker* markers, int* counts, int max_per_frame) {
    if (!c || !h_bgr || n_frames < 1 || height < 1 || row_stride < 1) return OCVAR_E_ARG;
    if ((long long)row_stride < (long long)format_bpp(c->input_format) * width) return OCVAR_E_ARG;
    // (the device slots keep the caller's strides, so the frame kernel's addressing limit is the host frames' too: refused here,
    // before anything is staged, not by the first sub-batch's enqueue after its upload)
    if (int rc = frame_span_check(c, width, height, row_stride, c->input_format)) return rc;
    // a grey frame is its own grey: no write-back kernel, no copy back, no page-locked buffers for it
    grey_in_place = grey_in_place && c->input_format != OCVAR_FMT_GRAY;
    if (n_frames > 1 && frame_stride < (size_t)height * row_stride) return OCVAR_E_ARG;
    if (!counts || max_per_frame < 0 || (max_per_frame > 0 && !markers)) return OCVAR_E_ARG;
    if (int rc = refuse_if_pending(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t frame_bytes = (size_t)height * row_stride;
    const size_t bytes = (size_t)(n_frames - 1) * frame_stride + frame_bytes;
    const int sub = c->ws.max_batch < HOST_SUB_BATCH ? c->ws.max_batch : HOST_SUB_BATCH;
    const int n_sub = (n_frames + sub - 1) / sub;
    struct Span { size_t off, len; int cnt; };   // a sub-batch: byte offset in the caller's buffer, bytes, frames
    auto span = [&](int k) {
        const int cnt = (k + 1) * sub <= n_frames ? sub : n_frames - k * sub;
        return Span{(size_t)k * sub * frame_stride, (size_t)(cnt - 1) * frame_stride + frame_bytes, cnt};
    };
    const size_t span_max = (size_t)((n_frames < sub ? n_frames : sub) - 1) * frame_stride + frame_bytes;
    const bool direct = caller_pinned(h_bgr, bytes);
    HIP_TRY(c, c->d_frames.reserve(2 * span_max + 256));   // two device slots (256-byte aligned)
    const size_t slot_bytes = (span_max + 255) & ~(size_t)255;
    if (!direct)
        for (auto& b : c->h_stage) HIP_TRY(c, b.reserve(span_max));
    if (!direct && grey_in_place)
        for (auto& b : c->h_grey) HIP_TRY(c, b.reserve(span_max));
    HIP_TRY(c, c->h2d_stream.ensure(hipStreamNonBlocking));
    HIP_TRY(c, c->d2h_stream.ensure(hipStreamNonBlocking));
    for (auto& e : c->h2d_done) HIP_TRY(c, e.ensure(hipEventDisableTiming));
    // On any failure: nothing of this call may still be in flight when it returns (the staging buffers are reused by the next)
    std::thread* copier_ref = nullptr;   // (set once the helper thread exists: fail() must not leave it running)
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(c->h2d_stream);
        (void)hipStreamSynchronize(c->d2h_stream);
        (void)hipStreamSynchronize(c->stream);
        if (copier_ref && copier_ref->joinable()) copier_ref->join();
        c->pending = false;
        c->board_out_off = 0;
        c->board_out_valid = false;
        return code;
    };
#define HIP_TRY_HOST(expr)                                            \
    do {                                                              \
        hipError_t e_ = (expr);                                       \
        if (e_ != hipSuccess) {                                       \
            c->err = std::string(#expr) + ": " + hipGetErrorString(e_); \
            return fail(OCVAR_E_HIP);                                 \
        }                                                             \
    } while (0)
    // slot k & 1 (host and device) carries sub-batch k
    auto upload = [&](int k) -> hipError_t {
        const Span sp = span(k);
        const uint8_t* src = h_bgr + sp.off;
        if (!direct) {
            host_copy(c->h_stage[k & 1], src, sp.len);
            src = c->h_stage[k & 1];
        }
        hipError_t e = hipMemcpyAsync(c->d_frames + (size_t)(k & 1) * slot_bytes, src, sp.len, hipMemcpyHostToDevice, c->h2d_stream);
        if (e == hipSuccess) e = hipEventRecord(c->h2d_done[k & 1], c->h2d_stream);
        return e;
    };
    // the grey frames of sub-batch k, already on their way: wait for the copy engine, then a helper thread copies them from the
    // staging buffer into the caller's frames while this thread stages the next upload (different buffers)
    std::thread grey_copier;
    copier_ref = &grey_copier;
    auto grey_join = [&] { if (grey_copier.joinable()) grey_copier.join(); };
    auto grey_home = [&](int k) -> hipError_t {
        const hipError_t e = hipStreamSynchronize(c->d2h_stream);
        if (e != hipSuccess || direct) return e;
        const size_t len = span(k).len;
        grey_join();
        uint8_t* dst = h_bgr + span(k).off;
        const uint8_t* src = c->h_grey[k & 1];
        try {
            grey_copier = std::thread([=] { host_copy(dst, src, len); });
        } catch (...) {
            host_copy(dst, src, len);
        }
        return hipSuccess;
    };
    HIP_TRY_HOST(upload(0));
    for (int k = 0; k < n_sub; k++) {
        const Span sp = span(k);
        uint8_t* d_slot = c->d_frames + (size_t)(k & 1) * slot_bytes;
        HIP_TRY_HOST(hipStreamWaitEvent(c->stream, c->h2d_done[k & 1], 0));
        int rc = enqueue_impl(c, BatchRequest{d_slot, width, height, row_stride, frame_stride, sp.cnt, grey_in_place,
                                              prev ? prev + (size_t)k * sub * c->ws.maxm : nullptr,
                                              prev_counts ? prev_counts + k * sub : nullptr, false, c->input_format, 3},
                              c->stream, nullptr);
        if (rc) return fail(rc);
        // while sub-batch k computes: bring sub-batch k-1's grey home, then stage sub-batch k+1 into the slot it leaves
        if (k > 0 && grey_in_place) HIP_TRY_HOST(grey_home(k - 1));
        if (k + 1 < n_sub) HIP_TRY_HOST(upload(k + 1));
        c->board_out_off = k * sub;
        rc = ocvar_hip_collect(c, markers ? markers + (size_t)k * sub * max_per_frame : nullptr, counts + k * sub, max_per_frame);
        c->board_out_off = 0;
        if (rc) return fail(rc);
        if (grey_in_place)   // (the kernels of sub-batch k have finished: collect waited for them)
            // (slot k & 1 last held sub-batch k - 2, whose copy-back thread was joined when sub-batch k - 1's was started)
            HIP_TRY_HOST(hipMemcpyAsync(direct ? h_bgr + sp.off : c->h_grey[k & 1].p, d_slot, sp.len, hipMemcpyDeviceToHost, c->d2h_stream));
    }
    if (grey_in_place) HIP_TRY_HOST(grey_home(n_sub - 1));
    grey_join();
#undef HIP_TRY_HOST
    return OCVAR_OK;
}

extern "C" int ocvar_hip_find_squares(OcvarHip* c, const uint8_t* h_gray, int width, int height, int row_stride, int* quads,
                                      int max_quads, int* n_quads) {
    if (!c || !h_gray || !quads || !n_quads || width < 16 || height < 16 || row_stride < width) return OCVAR_E_ARG;
    if (width > c->ws.max_w || height > c->ws.max_h) return OCVAR_E_ARG;   // (before the expanded copy is made, not after)
    if (int rc = frame_span_check(c, width, height, 3 * width, OCVAR_FMT_BGR)) return rc;
    std::vector<uint8_t> bgr((size_t)width * height * 3);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const uint8_t g = h_gray[(size_t)y * row_stride + x];
            uint8_t* p = &bgr[((size_t)y * width + x) * 3];
            p[0] = p[1] = p[2] = g;  // grey of an equal-channel pixel is the pixel
        }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = stage_frames(c, bgr.data(), height, width * 3, (size_t)width * height * 3, 1);
    if (rc) return rc;
    // (the expanded image, whatever the context's input format)
    rc = enqueue_impl(c, BatchRequest{c->d_frames, width, height, width * 3, (size_t)width * height * 3, 1, 0, nullptr, nullptr, false,
                                      OCVAR_FMT_BGR, 2},
                      c->stream, nullptr);
    if (rc) return rc;
    rc = wait_impl(c);
    if (rc) return rc;
    return quads_to_host(c, 0, max_quads < c->ws.maxq ? max_quads : c->ws.maxq, quads, n_quads);
}
