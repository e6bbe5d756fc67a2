// refine_registration_driver.cpp -- an application of the reference's API that turns on the corner refinement extension
// (cvarSetCornerRefine) of libopencv-ar.so and then calls cvarArMultRegistration over a short video, carrying its markers
// from frame to frame, for tests/test_gpu_corner_refine.py.  TEST ONLY.
//   refine_registration_driver <in> <out> <half_win> <max_iter> <eps>
//   in:  int width, height, n_templates, n_frames; CvarTemplate[n]; CvarCamera; n_frames BGR frames (width * 3 per row)
//   out: per frame: int count, n_out; CvarMarker[n_out]
#include "opencvar/opencvar.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    cvarSetCornerRefine(std::atoi(argv[3]), std::atoi(argv[4]), std::atof(argv[5]));
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[4];
    if (std::fread(hdr, sizeof hdr, 1, f) != 1) return 2;
    vector<CvarTemplate> templates(hdr[2]);
    CvarCamera camera;
    if ((hdr[2] && std::fread(templates.data(), sizeof(CvarTemplate), hdr[2], f) != (size_t)hdr[2]) ||
        std::fread(&camera, sizeof camera, 1, f) != 1)
        return 2;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::vector<char> bgr((size_t)hdr[0] * hdr[1] * 3);
    vector<CvarMarker> markers;
    for (int t = 0; t < hdr[3]; t++) {
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
