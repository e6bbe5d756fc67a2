"""CPU tests of the input-format setting (include/ocvar_hip.h: ocvar_hip_set_input_format): the declarations, the exported
symbols, the Python wrappers' format names, default strides and shape checks, the setters' NULL handling, and the frame
kernel's grey coefficients over every (b, g, r) triple.  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_kit as FK
import helpers as H

HEADER_FORMATS = {"OCVAR_FMT_" + name.upper(): code for name, code in FK.FORMATS.items()}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    import opencv_ar_amd
    return opencv_ar_amd


def _header(name):
    return open(os.path.join(H.ROOT, "include", name)).read()


def test_headers_declare_the_setters_and_the_formats():
    hip = _header("ocvar_hip.h")
    for name in ("ocvar_hip_set_input_format", "ocvar_hip_pipe_set_input_format"):
        assert re.search(r"\bint\s+%s\s*\(\s*Ocvar\w+\*\s*\w+\s*,\s*int\s+format\s*\)\s*;" % name, hip), name
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(OCVAR_FMT_\w+)\s*=\s*(\d+)", hip))
    assert enum == HEADER_FORMATS
    multi = _header("ocvar_multi.h")
    inc = re.findall(r'#include\s+"(ocvar_multi\w*\.h)"', multi)
    decl = "".join(_header(x) for x in inc)
    assert re.search(r"\bint\s+ocvar_multi_set_input_format\s*\(\s*OcvarMulti\*\s*m\s*,\s*int\s+format\s*\)\s*;", decl)


def test_libraries_export_the_setters(pkg):
    lib = pkg.hip_lib()
    assert hasattr(lib, "ocvar_hip_set_input_format") and hasattr(lib, "ocvar_hip_pipe_set_input_format")
    assert "ocvar_hip_set_input_format" in pkg.HIP_SYMBOLS and "ocvar_hip_pipe_set_input_format" in pkg.HIP_SYMBOLS
    multi = C.CDLL(os.path.join(pkg.LIB_DIR, "libocvar_multi.so"))
    assert hasattr(multi, "ocvar_multi_set_input_format")


def test_setters_refuse_a_null_context(pkg):
    lib = pkg.hip_lib()
    multi = C.CDLL(os.path.join(pkg.LIB_DIR, "libocvar_multi.so"))
    multi.ocvar_multi_set_input_format.argtypes = [C.c_void_p, C.c_int]
    for fmt in (0, 4, 9):
        assert lib.ocvar_hip_set_input_format(None, fmt) == -2
        assert lib.ocvar_hip_pipe_set_input_format(None, fmt) == -2
        assert multi.ocvar_multi_set_input_format(None, fmt) == -2


def test_format_names_and_bytes_per_pixel(pkg):
    assert {k: pkg.input_format_code(k) for k in pkg.INPUT_FORMATS} == {"bgr": 0, "rgb": 1, "bgra": 2, "rgba": 3, "gray": 4}
    assert pkg.input_format_code("GRAY") == 4 and pkg.input_format_code(2) == 2
    assert pkg.FORMAT_BPP == {0: 3, 1: 3, 2: 4, 3: 4, 4: 1}
    for bad in ("yuv", "grey", 5, -1, None, True):
        with pytest.raises(ValueError):
            pkg.input_format_code(bad)


def test_host_frame_shapes_must_match_the_format(pkg):
    assert pkg.frame_shape_bpp((2, 48, 64), "gray") == (2, 48, 64)
    assert pkg.frame_shape_bpp((2, 48, 64, 3), "bgr") == (2, 48, 64)
    assert pkg.frame_shape_bpp((2, 48, 64, 3), "rgb") == (2, 48, 64)
    assert pkg.frame_shape_bpp((2, 48, 64, 4), "rgba") == (2, 48, 64)
    for shape, fmt in (((2, 48, 64, 3), "gray"), ((2, 48, 64), "bgr"), ((2, 48, 64, 3), "bgra"), ((2, 48, 64, 4), "rgb"),
                       ((2, 48, 64, 1), "gray")):
        with pytest.raises(ValueError):
            pkg.frame_shape_bpp(shape, fmt)


class _Recorder:
    """stands in for the C library: records the arguments of the calls the wrappers make"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_default_strides_follow_the_format(pkg):
    w, h = 64, 48
    for fmt, bpp in (("bgr", 3), ("rgb", 3), ("bgra", 4), ("rgba", 4), ("gray", 1)):
        det = pkg.Detector.__new__(pkg.Detector)
        det._lib, det._ctx, det.input_format = _Recorder(), C.c_void_p(1), 0
        det.set_input_format(fmt)
        det.enqueue_device(1234, w, h, 2)
        frames = np.zeros((2, h, w) if bpp == 1 else (2, h, w, bpp), np.uint8)
        det.detect_host(frames)
        pipe = pkg.Pipe.__new__(pkg.Pipe)
        pipe._lib, pipe._p, pipe.input_format, pipe.chunk_frames = _Recorder(), C.c_void_p(1), 0, 4
        pipe.set_input_format(fmt)
        pipe.detect_device(1234, w, h, 2)
        pipe.submit(1234, w, h, 2)
        pipe.track_device(1234, w, h, 2)
        calls = dict(det._lib.calls)
        assert calls["ocvar_hip_set_input_format"][1] == pkg.INPUT_FORMATS[fmt]
        assert calls["ocvar_hip_enqueue"][4:6] == (bpp * w, bpp * w * h), fmt
        assert calls["ocvar_hip_detect_host"][2:6] == (w, h, bpp * w, bpp * w * h), fmt
        pcalls = dict(pipe._lib.calls)
        assert pcalls["ocvar_hip_pipe_set_input_format"][1] == pkg.INPUT_FORMATS[fmt]
        for name in ("ocvar_hip_pipe_detect_device", "ocvar_hip_pipe_submit", "ocvar_hip_pipe_track_device"):
            assert pcalls[name][4:6] == (bpp * w, bpp * w * h), (fmt, name)
        det._ctx = pipe._p = None   # (nothing to destroy)


def _coefficients():
    src = open(os.path.join(H.PKG, "csrc", "hd.h")).read()
    vals = {}
    for name in ("GREY_KH_BGR", "GREY_KL_BGR", "GREY_KH_RGB", "GREY_KL_RGB"):
        m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, src)
        assert m, name
        vals[name] = eval(m.group(1).replace("u", ""), {})   # e.g. 29u | (150u << 8) | (76u << 16)
    return vals


def test_split_coefficients_give_bgr2gray_for_both_byte_orders():
    """(dot4(pixel, KH) << 8) + dot4(pixel, KL) + 32768, byte 2, equals (1868 B + 9617 G + 4899 R + 8192) >> 14 for all 2^24
    pixels, in B G R x order with the BGR words and in R G B x order with the RGB words; byte 3 (alpha) has weight 0"""
    k = _coefficients()

    def split(word):
        return [(word >> (8 * j)) & 255 for j in range(4)]

    g = np.arange(256, dtype=np.int64)[:, None]
    r = np.arange(256, dtype=np.int64)[None, :]
    for hi, lo, rev in ((k["GREY_KH_BGR"], k["GREY_KL_BGR"], False), (k["GREY_KH_RGB"], k["GREY_KL_RGB"], True)):
        kh, kl = split(hi), split(lo)
        assert kh[3] == 0 and kl[3] == 0
        for b in range(256):
            want = (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14
            p = (r, g, b) if rev else (b, g, r)   # bytes 0, 1, 2 of the pixel
            s = ((kh[0] * p[0] + kh[1] * p[1] + kh[2] * p[2]) << 8) + kl[0] * p[0] + kl[1] * p[1] + kl[2] * p[2] + 32768
            assert np.array_equal((s >> 16) & 255, want), (rev, b)
