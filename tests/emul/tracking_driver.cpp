// tracking_driver.cpp -- a video loop over cvarArMultRegistration of libopencv-ar.so, the `markers` vector carried from call
// to call as an application built on the reference keeps it (samples/ARTest.cpp), for tests/test_gpu_dense.py.  TEST ONLY.
// One process = one fresh library context.
//   tracking_driver <in> <out>
//   in:  int width, height, n_templates, n_steps, n_in; CvarTemplate[n_templates]; CvarCamera; CvarMarker[n_in] (the vector
//        before the first call); n_steps BGR frames (width * 3 per row)
//   out: per step: int count, n_out; CvarMarker[n_out]
#include "opencvar/opencvar.h"
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[5];
    if (std::fread(hdr, sizeof hdr, 1, f) != 1) return 2;
    vector<CvarTemplate> templates(hdr[2]);
    CvarCamera camera;
    vector<CvarMarker> markers(hdr[4]);
    if ((hdr[2] && std::fread(templates.data(), sizeof(CvarTemplate), hdr[2], f) != (size_t)hdr[2]) ||
        std::fread(&camera, sizeof camera, 1, f) != 1 ||
        (hdr[4] && std::fread(markers.data(), sizeof(CvarMarker), hdr[4], f) != (size_t)hdr[4]))
        return 2;
    std::vector<char> bgr((size_t)hdr[0] * hdr[1] * 3);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int s = 0; s < hdr[3]; s++) {
        if (std::fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) return 2;
        IplImage img;
        std::memset(&img, 0, sizeof img);
        img.nSize = sizeof img;
        img.nChannels = 3;
        img.depth = IPL_DEPTH_8U;
        img.width = hdr[0];
        img.height = hdr[1];
        img.widthStep = hdr[0] * 3;
        img.imageSize = img.widthStep * img.height;
        img.imageData = img.imageDataOrigin = bgr.data();
        const int count = cvarArMultRegistration(&img, &markers, templates, &camera);
        const int out[2] = {count, (int)markers.size()};
        std::fwrite(out, sizeof out, 1, o);
        if (!markers.empty()) std::fwrite(markers.data(), sizeof(CvarMarker), markers.size(), o);
    }
    std::fclose(f);
    std::fclose(o);
    return 0;
}
