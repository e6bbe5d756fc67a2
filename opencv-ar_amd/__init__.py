"""MI355X-native AR-marker detection path of youtalk/opencv-ar -- Python binding of the C ABI.

The product is `lib/libocvar_hip.so` (hand-written HIP kernels for gfx950 behind `include/ocvar_hip.h`) and
`lib/libopencv-ar.so` (the host C++ mirror of the reference's `include/opencvar` API).  This module only binds
the C ABI with ctypes so that tests, `bench.py` and Python callers can drive it; torch is used by callers for
device memory and `torch.distributed`, never for compute.  There is no CPU fallback: importing works without a
GPU (so the symbol table can be checked), creating a `Detector` does not.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
HIP_LIB = os.environ.get("OCVAR_HIP_LIB") or os.path.join(LIB_DIR, "libocvar_hip.so")   # (override: instrumented builds of tools/prof_tier2.py)
SYNTH_LIB = os.path.join(LIB_DIR, "libocvar_synth.so")
HOST_LIB = os.path.join(LIB_DIR, "libopencv-ar.so.1.0.0")

MAX_TEMPLATES, MAX_TEMPLATE_SIZES, MAX_QUADS, MAX_MARKERS = 4096, 16, 256, 64
MAX_QUADS_EX, MAX_QUADS_DENSE, MAX_MARKERS_DENSE = 1792, 16384, 4096   # ocvar_hip_create_ex / ocvar_hip_create_dense limits

# every symbol include/ocvar_hip.h declares
HIP_SYMBOLS = [
    "ocvar_hip_create", "ocvar_hip_create_ex", "ocvar_hip_create_dense", "ocvar_hip_max_markers", "ocvar_hip_capacity_flags", "ocvar_hip_gate_create", "ocvar_hip_gate_create_lanes", "ocvar_hip_gate_lanes", "ocvar_hip_gate_destroy", "ocvar_hip_set_gate", "ocvar_hip_ready", "ocvar_hip_set_result_limit",
    "ocvar_hip_pipe_create", "ocvar_hip_pipe_destroy", "ocvar_hip_pipe_last_error", "ocvar_hip_pipe_set_templates", "ocvar_hip_pipe_set_camera",
    "ocvar_hip_pipe_detect_device", "ocvar_hip_pipe_track_device", "ocvar_hip_pipe_submit", "ocvar_hip_pipe_collect", "ocvar_hip_pipe_in_flight", "ocvar_hip_pipe_set_result_limit", "ocvar_hip_set_input_format", "ocvar_hip_pipe_set_input_format", "ocvar_hip_set_corner_refine", "ocvar_hip_pipe_set_corner_refine", "ocvar_hip_enqueue_tracked", "ocvar_hip_build_info", "ocvar_hip_set_tuning", "ocvar_hip_destroy", "ocvar_hip_last_error", "ocvar_hip_set_templates", "ocvar_hip_set_camera",
    "ocvar_hip_detect_device", "ocvar_hip_enqueue", "ocvar_hip_collect", "ocvar_hip_detect_host", "ocvar_hip_find_squares",
    "ocvar_hip_debug_gray", "ocvar_hip_debug_binary", "ocvar_hip_debug_masks", "ocvar_hip_debug_frame_quads", "ocvar_hip_debug_candidates",
    "ocvar_hip_debug_crop_rois", "ocvar_hip_debug_crop_plane", "ocvar_hip_debug_starts", "ocvar_hip_debug_rings",
    "ocvar_hip_stage_ms", "ocvar_hip_stream", "ocvar_hip_stage_stamps", "ocvar_hip_counters", "ocvar_hip_results_to_device", "ocvar_hip_results_to_device_ex", "ocvar_hip_debug_calibrate",
    "ocvar_hip_set_board", "ocvar_hip_board_poses", "ocvar_hip_board_poses_to_device",
    "ocvar_hip_set_overlay", "ocvar_hip_render", "ocvar_hip_render_records",
    "ocvar_hip_annotate_default_style", "ocvar_hip_annotate", "ocvar_hip_annotate_records",
    "ocvar_hip_patches", "ocvar_hip_patches_records",
    "ocvar_hip_undistort", "ocvar_hip_undistort_records",
    "ocvar_hip_flow_records",
    "ocvar_hip_yuv_to_frames", "ocvar_hip_frames_to_yuv", "ocvar_hip_yuv_to_frames_ex", "ocvar_hip_frames_to_yuv_ex",
    "ocvar_hip_resize", "ocvar_hip_scale_records",
    "ocvar_hip_orient", "ocvar_hip_orient_records", "ocvar_hip_orient_camera",
    "ocvar_hip_warp", "ocvar_hip_warp_records", "ocvar_hip_board_plane_maps",
    "ocvar_hip_levels_default_params", "ocvar_hip_levels",
    "ocvar_hip_bayer_default_params", "ocvar_hip_bayer_pattern_at", "ocvar_hip_bayer_to_frames",
]
# input formats (include/ocvar_hip.h: OCVAR_FMT_*) and their bytes per pixel
INPUT_FORMATS = {"bgr": 0, "rgb": 1, "bgra": 2, "rgba": 3, "gray": 4}
FORMAT_BPP = {0: 3, 1: 3, 2: 4, 3: 4, 4: 1}


def input_format_code(fmt):
    """'bgr' | 'rgb' | 'bgra' | 'rgba' | 'gray' (or the OCVAR_FMT_* value) -> the OCVAR_FMT_* value"""
    if isinstance(fmt, str) and fmt.lower() in INPUT_FORMATS:
        return INPUT_FORMATS[fmt.lower()]
    if isinstance(fmt, int) and not isinstance(fmt, bool) and fmt in FORMAT_BPP:
        return fmt
    raise ValueError(f"unknown input format {fmt!r}: one of {sorted(INPUT_FORMATS)}")


def frame_shape_bpp(shape, fmt):
    """(n, h, w) of a host frame array [n, H, W] (gray) or [n, H, W, bpp] in format fmt; ValueError if the shape does not fit"""
    bpp = FORMAT_BPP[input_format_code(fmt)]
    if bpp == 1:
        if len(shape) != 3:
            raise ValueError(f"gray frames are [n, H, W], got {tuple(shape)}")
    elif len(shape) != 4 or shape[3] != bpp:
        raise ValueError(f"frames in this format are [n, H, W, {bpp}], got {tuple(shape)}")
    return shape[0], shape[1], shape[2]


MAX_REFINE_HALF_WIN = 15   # include/ocvar_hip.h: OCVAR_MAX_REFINE_HALF_WIN


def corner_refine_args(half_win, max_iter, eps):
    """(half_win, max_iter, eps) of a corner refinement setting, checked: ValueError outside half_win 0..15 (0: off),
    max_iter 1..100, eps >= 0"""
    for name, v in (("half_win", half_win), ("max_iter", max_iter)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an int, got {v!r}")
    if not 0 <= half_win <= MAX_REFINE_HALF_WIN:
        raise ValueError(f"half_win must be 0 .. {MAX_REFINE_HALF_WIN}, got {half_win}")
    if not 1 <= max_iter <= 100:
        raise ValueError(f"max_iter must be 1 .. 100, got {max_iter}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not 0 <= float(eps) < 1e30:
        raise ValueError(f"eps must be a number >= 0, got {eps!r}")
    return int(half_win), int(max_iter), float(eps)


MAX_BOARD_MARKERS = 256   # include/ocvar_hip.h: OCVAR_MAX_BOARD_MARKERS
MAX_OVERLAYS, MAX_OVERLAY_SIDE = 64, 1024   # include/ocvar_hip.h: OCVAR_MAX_OVERLAYS, OCVAR_MAX_OVERLAY_SIDE
MAX_PATCH_SIDE, PATCH_FLIP_ROWS, PATCH_MATCHED_ONLY = 256, 1, 2   # include/ocvar_hip.h: OCVAR_MAX_PATCH_SIDE, OCVAR_PATCH_*
MAX_FLOW_HALF_WIN, MAX_FLOW_LEVELS, FLOW_POSE = 15, 5, 1   # include/ocvar_hip.h: OCVAR_MAX_FLOW_HALF_WIN, OCVAR_MAX_FLOW_LEVELS, OCVAR_FLOW_POSE


class FlowParams(C.Structure):  # OcvarFlowParams
    _fields_ = [("half_win", C.c_int), ("levels", C.c_int), ("max_iter", C.c_int), ("flags", C.c_int),
                ("eps", C.c_float), ("min_eig", C.c_float), ("max_err", C.c_float), ("fb_max", C.c_float)]


def flow_params(half_win=10, levels=3, max_iter=30, eps=0.03, min_eig=1e-3, max_err=0.0, fb_max=0.0, pose=False):
    """The parameters of Detector.flow_records (include/ocvar_hip.h: OcvarFlowParams; the defaults are the library's), checked:
    ValueError outside half_win 1..15, levels 0..5, max_iter 1..100, or for a negative or non-finite eps, min_eig, max_err, fb_max"""
    for name, v, lo, hi in (("half_win", half_win, 1, MAX_FLOW_HALF_WIN), ("levels", levels, 0, MAX_FLOW_LEVELS), ("max_iter", max_iter, 1, 100)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an int in {lo} .. {hi}, got {v!r}")
    for name, v in (("eps", eps), ("min_eig", min_eig), ("max_err", max_err), ("fb_max", fb_max)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= float(v) < 3e38:
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    return FlowParams(int(half_win), int(levels), int(max_iter), FLOW_POSE if pose else 0, float(eps), float(min_eig), float(max_err), float(fb_max))


# include/ocvar_hip.h: OCVAR_ANNO_*
ANNO_OUTLINE, ANNO_CORNER0, ANNO_AXES, ANNO_CUBE, ANNO_LABEL, ANNO_UNMATCHED, ANNO_COLOR_BY_TEMPLATE = 1, 2, 4, 8, 16, 32, 64
ANNO_MAX_THICKNESS, ANNO_MAX_LABEL_SCALE, ANNO_MAX_COORD, ANNO_RECORD_BYTES = 16, 8, 1048576, 696
ANNO_FLAG_NAMES = {"outline": ANNO_OUTLINE, "corner0": ANNO_CORNER0, "axes": ANNO_AXES, "cube": ANNO_CUBE, "label": ANNO_LABEL,
                   "unmatched": ANNO_UNMATCHED, "color_by_template": ANNO_COLOR_BY_TEMPLATE}
ANNO_COLOUR_NAMES = ("outline_color", "unmatched_color", "corner0_color", "cube_color", "label_color")


class AnnotateStyle(C.Structure):  # OcvarAnnotateStyle
    _fields_ = [("flags", C.c_int), ("thickness", C.c_int), ("label_scale", C.c_int), ("reserved", C.c_int),
                ("axis_length", C.c_double), ("cube_height", C.c_double),
                ("outline", C.c_uint8 * 4), ("unmatched", C.c_uint8 * 4), ("corner0", C.c_uint8 * 4), ("cube", C.c_uint8 * 4),
                ("label", C.c_uint8 * 4), ("reserved2", C.c_uint8 * 4)]


def annotate_style(**kw):
    """The style of Detector.annotate / annotate_records (include/ocvar_hip.h: OcvarAnnotateStyle), starting from the library's
    defaults (ocvar_hip_annotate_default_style): flags as keyword booleans outline, corner0, axes, cube, label, unmatched,
    color_by_template; thickness (1 .. 16), label_scale (0: automatic, .. 8), axis_length, cube_height (finite, >= 0); colours
    outline_color, unmatched_color, corner0_color, cube_color, label_color as (R, G, B, A) of 0 .. 255.  ValueError for an unknown
    keyword or a value outside its range."""
    st = AnnotateStyle()
    if hip_lib().ocvar_hip_annotate_default_style(C.byref(st)) != 0:
        raise OcvarError("ocvar_hip_annotate_default_style failed")
    for name, v in kw.items():
        if name in ANNO_FLAG_NAMES:
            st.flags = (st.flags | ANNO_FLAG_NAMES[name]) if v else (st.flags & ~ANNO_FLAG_NAMES[name])
        elif name in ("thickness", "label_scale"):
            lo, hi = (1, ANNO_MAX_THICKNESS) if name == "thickness" else (0, ANNO_MAX_LABEL_SCALE)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an int in {lo} .. {hi}, got {v!r}")
            setattr(st, name, int(v))
        elif name in ("axis_length", "cube_height"):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= float(v) < float("inf"):
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
            setattr(st, name, float(v))
        elif name in ANNO_COLOUR_NAMES:
            c = tuple(v)
            if len(c) != 4 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= x <= 255 for x in c):
                raise ValueError(f"{name} must be (R, G, B, A) of 0 .. 255, got {v!r}")
            getattr(st, name[:-len("_color")])[:] = [int(x) for x in c]
        else:
            raise ValueError(f"unknown style keyword {name!r}")
    if not st.flags & (ANNO_OUTLINE | ANNO_CORNER0 | ANNO_AXES | ANNO_CUBE | ANNO_LABEL):
        raise ValueError("a style draws at least one of outline, corner0, axes, cube and label")
    return st


YUV_LAYOUTS = {"nv12": 0, "i420": 1, "yuyv": 2, "uyvy": 3}   # include/ocvar_hip.h: OCVAR_YUV_NV12 ..
YUV_MATRICES = {"bt601": 0, "bt709": 1}                      # include/ocvar_hip.h: OCVAR_YUV_BT601, OCVAR_YUV_BT709
# what OcvarYuvFramesEx takes (YuvFramesEx): the above and OCVAR_YUV_NV21, _I444; OCVAR_YUV_BT2020; OCVAR_YUV_LIMITED, _FULL; the depths
YUV_EX_LAYOUTS = {"nv12": 0, "i420": 1, "yuyv": 2, "uyvy": 3, "nv21": 4, "i444": 5}
YUV_EX_MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}
YUV_RANGES = {"limited": 0, "full": 1}
YUV_BITS = (8, 10, 12, 16)
RESIZE_INTERPS = {"nearest": 0, "linear": 1, "area": 2}     # include/ocvar_hip.h: OCVAR_RESIZE_NEAREST ..
SCALE_POSE = 1                                              # include/ocvar_hip.h: OCVAR_SCALE_POSE
# include/ocvar_hip.h: OCVAR_ORIENT_IDENTITY ..; a pixel (x, y) of a W x H frame goes to (x, y), (H-1-y, x), (W-1-x, H-1-y), (y, W-1-x),
# (W-1-x, y), (x, H-1-y), (y, x), (H-1-y, W-1-x)
ORIENTATIONS = {"identity": 0, "rot90": 1, "rot180": 2, "rot270": 3, "flip_h": 4, "flip_v": 5, "transpose": 6, "transverse": 7}
ORIENT_POSE = 1                                             # include/ocvar_hip.h: OCVAR_ORIENT_POSE


WARP_INTERPS = {"nearest": 0, "linear": 1}                  # include/ocvar_hip.h: OCVAR_WARP_NEAREST, OCVAR_WARP_LINEAR
WARP_BORDERS = {"constant": 0, "replicate": 1}              # include/ocvar_hip.h: OCVAR_WARP_BORDER_*
WARP_INVERSE_MAP, WARP_ONE_MAP, WARP_POSE = 1, 2, 4         # include/ocvar_hip.h: OCVAR_WARP_INVERSE_MAP ..
LEVELS_MAX_TILES_AXIS, LEVELS_MAX_TILES, LEVELS_MAX_PPM = 16, 64, 500000   # include/ocvar_hip.h: OcvarLevelsParams' ranges


class LevelsParams(C.Structure):  # OcvarLevelsParams
    _fields_ = [("tiles_x", C.c_int), ("tiles_y", C.c_int), ("low_ppm", C.c_int), ("high_ppm", C.c_int), ("max_gain_q8", C.c_int)]


def levels_params(tiles=(1, 1), low_ppm=10000, high_ppm=10000, max_gain=8.0):
    """The parameters of Detector.levels (include/ocvar_hip.h: OcvarLevelsParams; the defaults are the library's), checked: tiles =
    (tiles_x, tiles_y) of 1 .. 16 each and at most 64 in all (that neither exceeds the frame's side is the call's to check), low_ppm
    and high_ppm the parts per million clipped at the dark and the bright end, 0 .. 500000, max_gain the largest gain, 1 .. 255
    (stored in 1/256).  ValueError outside those."""
    try:
        tx, ty = tiles
    except (TypeError, ValueError):
        raise ValueError(f"tiles must be (tiles_x, tiles_y), got {tiles!r}") from None
    for name, v, lo, hi in (("tiles_x", tx, 1, LEVELS_MAX_TILES_AXIS), ("tiles_y", ty, 1, LEVELS_MAX_TILES_AXIS),
                            ("low_ppm", low_ppm, 0, LEVELS_MAX_PPM), ("high_ppm", high_ppm, 0, LEVELS_MAX_PPM)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an int in {lo} .. {hi}, got {v!r}")
    if tx * ty > LEVELS_MAX_TILES:
        raise ValueError(f"at most {LEVELS_MAX_TILES} tiles, got {tx} x {ty}")
    if isinstance(max_gain, bool) or not isinstance(max_gain, (int, float, np.integer, np.floating)) or not 1.0 <= float(max_gain) <= 255.0:
        raise ValueError(f"max_gain must be a number in 1 .. 255, got {max_gain!r}")
    return LevelsParams(int(tx), int(ty), int(low_ppm), int(high_ppm), int(round(float(max_gain) * 256)))


BAYER_PATTERNS = {"rggb": 0, "grbg": 1, "gbrg": 2, "bggr": 3}   # include/ocvar_hip.h: OCVAR_BAYER_RGGB .. (the top-left 2 x 2, row by row)
BAYER_MAX_GAIN = 16383                                          # include/ocvar_hip.h: OcvarBayerParams' gains, 1024 = 1.0


class BayerParams(C.Structure):  # OcvarBayerParams
    _fields_ = [("pattern", C.c_int), ("bits", C.c_int), ("black", C.c_int), ("gain_b", C.c_int), ("gain_g", C.c_int), ("gain_r", C.c_int)]


def _bayer_pattern_code(pattern):
    if isinstance(pattern, str) and pattern.lower() in BAYER_PATTERNS:
        return BAYER_PATTERNS[pattern.lower()]
    if not isinstance(pattern, bool) and isinstance(pattern, (int, np.integer)) and int(pattern) in BAYER_PATTERNS.values():
        return int(pattern)
    raise ValueError(f"unknown Bayer pattern {pattern!r}: one of {sorted(BAYER_PATTERNS)}")


def bayer_params(pattern="rggb", bits=8, black=0, gains=(1.0, 1.0, 1.0)):
    """The parameters of Detector.bayer_to_frames (include/ocvar_hip.h: OcvarBayerParams; the defaults are the library's), checked:
    pattern a name of BAYER_PATTERNS (the colours of the top-left 2 x 2 block, row by row; OpenCV's COLOR_BayerBG2BGR is 'rggb') or
    its code, bits 8 .. 16 (8: bytes; more: 16-bit words, right-aligned), black 0 .. 2^bits - 1, gains = (blue, green, red) as
    numbers of 0 .. 16383 / 1024 (stored in 1/1024).  ValueError outside those."""
    code = _bayer_pattern_code(pattern)
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 8 <= bits <= 16:
        raise ValueError(f"bits must be an int in 8 .. 16, got {bits!r}")
    if isinstance(black, bool) or not isinstance(black, (int, np.integer)) or not 0 <= black <= (1 << int(bits)) - 1:
        raise ValueError(f"black must be an int in 0 .. {(1 << int(bits)) - 1}, got {black!r}")
    try:
        gb, gg, gr = gains
    except (TypeError, ValueError):
        raise ValueError(f"gains must be (blue, green, red), got {gains!r}") from None
    q = []
    for name, g in (("blue", gb), ("green", gg), ("red", gr)):
        if isinstance(g, bool) or not isinstance(g, (int, float, np.integer, np.floating)) or not 0 <= int(round(float(g) * 1024)) <= BAYER_MAX_GAIN:
            raise ValueError(f"the {name} gain must be a number in 0 .. {BAYER_MAX_GAIN / 1024:.3f}, got {g!r}")
        q.append(int(round(float(g) * 1024)))
    return BayerParams(code, int(bits), int(black), q[0], q[1], q[2])


def bayer_pattern_at(pattern, x0, y0):
    """the name of the pattern of a source rectangle whose origin is sample (x0, y0) of a mosaic in `pattern` (a name or a code):
    pass it with the pointer moved to that sample and the full frame's strides.  No device call."""
    code = hip_lib().ocvar_hip_bayer_pattern_at(_bayer_pattern_code(pattern), int(x0), int(y0))
    return {v: k for k, v in BAYER_PATTERNS.items()}[code]


def perspective_map(src_quad, dst_quad):
    """the nine float64 numbers (row by row, the last one 1) of the projective map that sends the four points of src_quad to
    the four points of dst_quad (4 x 2 each): OpenCV's getPerspectiveTransform, solved in float64 from the four point pairs.  As
    it stands it is the forward map Detector.warp takes for frames whose pixels move from src_quad to dst_quad.  ValueError when
    the pairs do not determine a map (three points of a quad on a line)."""
    s, d = np.asarray(src_quad, np.float64), np.asarray(dst_quad, np.float64)
    if s.shape != (4, 2) or d.shape != (4, 2):
        raise ValueError(f"perspective_map: two 4 x 2 quads, got {s.shape} and {d.shape}")
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k in range(4):
        x, y, u, v = s[k, 0], s[k, 1], d[k, 0], d[k, 1]
        A[2 * k] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        A[2 * k + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
        b[2 * k], b[2 * k + 1] = u, v
    try:
        h = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        raise ValueError("perspective_map: the four point pairs do not determine a map") from None
    if not np.isfinite(h).all():
        raise ValueError("perspective_map: the four point pairs do not determine a map")
    return np.append(h, 1.0)


def orientation_code(o):
    """'identity' | 'rot90' | 'rot180' | 'rot270' (clockwise) | 'flip_h' | 'flip_v' | 'transpose' | 'transverse' (or the
    OCVAR_ORIENT_* value) -> the OCVAR_ORIENT_* value"""
    if isinstance(o, str) and o.lower() in ORIENTATIONS:
        return ORIENTATIONS[o.lower()]
    if isinstance(o, (int, np.integer)) and not isinstance(o, bool) and int(o) in ORIENTATIONS.values():
        return int(o)
    raise ValueError(f"unknown orientation {o!r}: one of {list(ORIENTATIONS)}")


def orientation_inverse(o):
    """the orientation that undoes o: 'rot90' and 'rot270' undo each other, every other one undoes itself -> OCVAR_ORIENT_* value"""
    return {1: 3, 3: 1}.get(orientation_code(o), orientation_code(o))


def oriented_size(size, o):
    """(width, height) of the frames orientation o makes from frames of size = (width, height)"""
    return (size[1], size[0]) if orientation_code(o) in (1, 3, 6, 7) else (size[0], size[1])


def orientation_from_rotation(degrees):
    """the orientation that turns a frame by `degrees` clockwise (what a decoder reports as the rotation to apply for display): a
    multiple of 90, negative or beyond 360 included; ValueError otherwise"""
    if isinstance(degrees, bool) or not isinstance(degrees, (int, float, np.integer, np.floating)) or degrees != degrees or float(degrees) % 90 != 0:
        raise ValueError(f"a rotation must be a multiple of 90 degrees, got {degrees!r}")
    return int(float(degrees) // 90) % 4


def orientation_from_exif(tag):
    """the orientation that makes a picture stored under EXIF Orientation `tag` upright:
    1 identity, 2 flip_h, 3 rot180, 4 flip_v, 5 transpose, 6 rot90, 7 transverse, 8 rot270 (tag 6: row 0 of the stored picture is
    the visual right-hand side, so it is turned 90 degrees clockwise; tag 8: row 0 is the left-hand side); ValueError otherwise"""
    table = {1: 0, 2: 4, 3: 2, 4: 5, 5: 6, 6: 1, 7: 7, 8: 3}
    if isinstance(tag, bool) or not isinstance(tag, (int, np.integer)) or int(tag) not in table:
        raise ValueError(f"an EXIF orientation tag is 1 .. 8, got {tag!r}")
    return table[int(tag)]


def _yuv_code(table, what, v):
    if isinstance(v, str) and v.lower() in table:
        return table[v.lower()]
    if isinstance(v, int) and not isinstance(v, bool) and v in table.values():
        return v
    raise ValueError(f"unknown YUV {what} {v!r}: one of {sorted(table)}")


class YuvFrames(C.Structure):  # OcvarYuvFrames: where the planes of a block of YUV frames lie in device memory
    _fields_ = [("layout", C.c_int), ("matrix", C.c_int), ("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p),
                ("y_pitch", C.c_int), ("c_pitch", C.c_int), ("frame_stride", C.c_size_t)]

    @classmethod
    def from_surface(cls, ptr, width, height, layout, pitch=None, matrix="bt601"):
        """Frames whose planes follow each other without a gap, the way a decoder lays a surface out, frame after frame: 'nv12' --
        height rows of Y, then height / 2 rows of U V, all `pitch` bytes apart (default: width); 'i420' -- Y, then U, then V, the
        chroma rows pitch / 2 apart; 'yuyv' / 'uyvy' -- one plane, rows `pitch` apart (default: 2 * width).  For any other
        arrangement (a chroma offset, a gap between frames) fill the fields in directly."""
        code = _yuv_code(YUV_LAYOUTS, "layout", layout)
        m = _yuv_code(YUV_MATRICES, "matrix", matrix)
        if code in (0, 1):
            pitch = width if pitch is None else pitch
            if height % 2 or (code == 1 and pitch % 2):
                raise ValueError("4:2:0 surfaces have an even height, and an even pitch when planar")
            c_pitch = pitch if code == 0 else pitch // 2
            c0 = ptr + pitch * height
            c1 = c0 + c_pitch * (height // 2) if code == 1 else None
            return cls(code, m, ptr, c0, c1, pitch, c_pitch, pitch * height * 3 // 2)
        pitch = 2 * width if pitch is None else pitch
        return cls(code, m, ptr, None, None, pitch, 0, pitch * height)


class YuvFramesEx(C.Structure):  # OcvarYuvFramesEx: YuvFrames with a range, a depth, and the layouts and matrices of the _ex calls
    _fields_ = [("layout", C.c_int), ("matrix", C.c_int), ("range", C.c_int), ("bits", C.c_int), ("y", C.c_void_p), ("c0", C.c_void_p),
                ("c1", C.c_void_p), ("y_pitch", C.c_int), ("c_pitch", C.c_int), ("frame_stride", C.c_size_t)]

    @staticmethod
    def codes(layout, matrix="bt601", range="limited", bits=8):
        """(layout, matrix, range, bits) as the ABI's numbers; ValueError for what it refuses: an unknown name or number, a depth
        other than 8, 10, 12, 16, more than 8 bits with a layout other than 'nv12'"""
        code = _yuv_code(YUV_EX_LAYOUTS, "layout", layout)
        m = _yuv_code(YUV_EX_MATRICES, "matrix", matrix)
        r = _yuv_code(YUV_RANGES, "range", range)
        if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or int(bits) not in YUV_BITS:
            raise ValueError(f"YUV samples have {YUV_BITS} bits, got {bits!r}")
        if bits > 8 and code != 0:
            raise ValueError("more than 8 bits come as 'nv12' only (P010, P012, P016)")
        return code, m, r, int(bits)

    @classmethod
    def from_surface(cls, ptr, width, height, layout, pitch=None, matrix="bt601", range="limited", bits=8):
        """Frames whose planes follow each other without a gap, frame after frame, as YuvFrames.from_surface lays them out: 'nv12'
        and 'nv21' -- Y, then the interleaved chroma rows, all `pitch` bytes apart (default: width times the bytes of a sample; with
        bits 10, 12 or 16 'nv12' is P010, P012 or P016 and its pitch even); 'i420' -- Y, U, V, the chroma rows pitch / 2 apart;
        'i444' -- Y, U, V, all rows `pitch` apart; 'yuyv' / 'uyvy' -- one plane.  ValueError for what the ABI refuses of these
        parameters."""
        code, m, r, bits = cls.codes(layout, matrix, range, bits)
        sb = 2 if bits > 8 else 1
        if code in (2, 3):
            pitch = 2 * width if pitch is None else pitch
            return cls(code, m, r, bits, ptr, None, None, pitch, 0, pitch * height)
        pitch = width * sb if pitch is None else pitch
        if sb == 2 and (pitch % 2 or ptr % 2):
            raise ValueError("16-bit samples lie at even addresses, an even pitch apart")
        if code == 5:
            return cls(code, m, r, bits, ptr, ptr + pitch * height, ptr + 2 * pitch * height, pitch, pitch, 3 * pitch * height)
        if height % 2 or (code == 1 and pitch % 2):
            raise ValueError("4:2:0 surfaces have an even height, and an even pitch when planar")
        c_pitch = pitch // 2 if code == 1 else pitch
        c0 = ptr + pitch * height
        c1 = c0 + c_pitch * (height // 2) if code == 1 else None
        return cls(code, m, r, bits, ptr, c0, c1, pitch, c_pitch, pitch * height * 3 // 2)


class BoardMarker(C.Structure):  # OcvarBoardMarker: a template and the board-plane (z = 0) coordinates of its corners 0..3
    _fields_ = [("templateId", C.c_int), ("pad", C.c_int), ("corner", C.c_double * 8)]


# OcvarBoardPose: glMatrix (board frame -> GL modelview, as a marker record's), rvec / tvec (OpenCV: X_cam = R(rvec) X_board +
# tvec), rms (px), n_markers (board markers used), status (1 solved, 0 no board marker, -1 not solvable)
BOARD_DTYPE = np.dtype([("glMatrix", "<f8", (16,)), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("rms", "<f8"),
                        ("n_markers", "<i4"), ("status", "<i4")], align=True)
assert C.sizeof(BoardMarker) == 72 and BOARD_DTYPE.itemsize == 192


def grid_board(template_ids, cols, rows, length, separation):
    """A planar grid board (ArUco's GridBoard): marker k carries template_ids[k] and sits at column k % cols, row k // cols;
    its corners 0..3 are (x0, y0), (x0 + L, y0), (x0 + L, y0 + L), (x0, y0 + L) with x0 = col (L + s), y0 = row (L + s).
    Returns [(template_id, 4x2 corners)] for Detector.set_board."""
    if len(template_ids) > cols * rows:
        raise ValueError(f"{len(template_ids)} templates for a {cols} x {rows} grid")
    out = []
    for k, t in enumerate(template_ids):
        x0, y0 = (k % cols) * (length + separation), (k // cols) * (length + separation)
        out.append((int(t), np.array([[x0, y0], [x0 + length, y0], [x0 + length, y0 + length], [x0, y0 + length]], np.float64)))
    return out


STAGE_NAMES = ["binarise_frames", "follow1_frames", "follow2_frames", "follow3_frames", "order_crops", "binarise_crops",
               "follow1_crops", "follow2_crops", "follow3_crops", "decode", "dedupe_pose", "batch_total"]


class Camera(C.Structure):  # CvarCamera, reference include/opencvar/opencvar.h:54-60
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("cameraMatrix", C.c_double * 9),
                ("distCoeffs", C.c_double * 5), ("glProjection", C.c_double * 16)]


class Template(C.Structure):  # CvarTemplate, opencvar.h:65-70
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("scale", C.c_double), ("code", C.c_longlong * 4)]


class Marker(C.Structure):  # CvarMarker, opencvar.h:75-82
    _fields_ = [("glMatrix", C.c_double * 16), ("templateId", C.c_int), ("markerId", C.c_int),
                ("score", C.c_double), ("square", C.c_float * 8), ("aspectRatio", C.c_double)]


class Candidate(C.Structure):
    _fields_ = [("markerId", C.c_int), ("templateId", C.c_int), ("orient", C.c_int), ("valid", C.c_int),
                ("bit", C.c_longlong), ("square", C.c_float * 8), ("patPoint", C.c_float * 8)]


# OcvarCropRoi: a crop of the second pass (Detector.debug_crops)
CROP_ROI_DTYPE = np.dtype([(n, "<i4") for n in ("index", "frame", "owner", "x0", "y0", "w", "h")])
# OcvarStart: a border start of the frame or crop pass (Detector.debug_starts)
START_DTYPE = np.dtype([(n, "<i4") for n in ("roi", "x", "y", "is_hole")])

MARKER_DTYPE = np.dtype([("glMatrix", "<f8", (16,)), ("templateId", "<i4"), ("markerId", "<i4"), ("score", "<f8"),
                         ("square", "<f4", (8,)), ("aspectRatio", "<f8")], align=True)
assert C.sizeof(Camera) == 248 and C.sizeof(Template) == 48 and C.sizeof(Marker) == 184 and MARKER_DTYPE.itemsize == 184


class OcvarError(RuntimeError):
    pass


_hip = None


def hip_lib():
    """Loads the HIP library; raises if it has not been built (no silent fallback)."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise OcvarError(f"{HIP_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback for the detection path)")
        try:
            # torch ships its own HIP runtime; load it first so this library binds to the same one instead of
            # bringing a second runtime into the process (two runtimes cannot both own the device)
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(HIP_LIB)
        vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
        lib.ocvar_hip_create.argtypes = [C.POINTER(vp), i, i, i, i]
        lib.ocvar_hip_create_dense.argtypes = [C.POINTER(vp), i, i, i, i, i, i]
        lib.ocvar_hip_max_markers.argtypes = [vp]
        lib.ocvar_hip_destroy.argtypes = [vp]
        lib.ocvar_hip_gate_create.argtypes = [C.POINTER(vp), i, i]
        lib.ocvar_hip_gate_create_lanes.argtypes = [C.POINTER(vp), i, i, i]
        lib.ocvar_hip_gate_lanes.argtypes = [vp]
        lib.ocvar_hip_gate_destroy.argtypes = [vp]
        lib.ocvar_hip_gate_destroy.restype = None
        lib.ocvar_hip_set_gate.argtypes = [vp, vp]
        lib.ocvar_hip_ready.argtypes = [vp]
        lib.ocvar_hip_set_result_limit.argtypes = [vp, i]
        lib.ocvar_hip_pipe_create.argtypes = [C.POINTER(vp), i, i, i, i, i, i]
        lib.ocvar_hip_pipe_destroy.argtypes = [vp]
        lib.ocvar_hip_pipe_destroy.restype = None
        lib.ocvar_hip_pipe_last_error.argtypes = [vp]
        lib.ocvar_hip_pipe_last_error.restype = C.c_char_p
        lib.ocvar_hip_pipe_set_templates.argtypes = [vp, vp, i]
        lib.ocvar_hip_pipe_set_camera.argtypes = [vp, vp]
        lib.ocvar_hip_pipe_detect_device.argtypes = [vp, vp, i, i, i, sz, C.c_longlong, i, vp, vp, i]
        lib.ocvar_hip_pipe_track_device.argtypes = [vp, vp, i, i, i, sz, C.c_longlong, i, i, vp, vp, i]
        lib.ocvar_hip_pipe_submit.argtypes = [vp, vp, i, i, i, sz, i, i, C.c_longlong]
        lib.ocvar_hip_pipe_collect.argtypes = [vp, C.POINTER(C.c_longlong), vp, vp, i]
        lib.ocvar_hip_pipe_in_flight.argtypes = [vp]
        lib.ocvar_hip_pipe_set_result_limit.argtypes = [vp, i]
        lib.ocvar_hip_pipe_set_input_format.argtypes = [vp, i]
        lib.ocvar_hip_set_input_format.argtypes = [vp, i]
        lib.ocvar_hip_set_corner_refine.argtypes = [vp, i, i, C.c_float]
        lib.ocvar_hip_pipe_set_corner_refine.argtypes = [vp, i, i, C.c_float]
        lib.ocvar_hip_enqueue_tracked.argtypes = [vp, vp, i, i, i, sz, i, i, vp, vp, vp]
        lib.ocvar_hip_set_tuning.argtypes = [vp, i, i]
        lib.ocvar_hip_build_info.argtypes = []
        lib.ocvar_hip_build_info.restype = C.c_char_p
        lib.ocvar_hip_destroy.restype = None
        lib.ocvar_hip_last_error.argtypes = [vp]
        lib.ocvar_hip_last_error.restype = C.c_char_p
        lib.ocvar_hip_set_templates.argtypes = [vp, vp, i]
        lib.ocvar_hip_set_camera.argtypes = [vp, vp]
        lib.ocvar_hip_detect_device.argtypes = [vp, vp, i, i, i, sz, i, i, vp, vp, vp, vp, i]
        lib.ocvar_hip_enqueue.argtypes = [vp, vp, i, i, i, sz, i, i, vp, vp, vp]
        lib.ocvar_hip_collect.argtypes = [vp, vp, vp, i]
        lib.ocvar_hip_detect_host.argtypes = [vp, vp, i, i, i, sz, i, i, vp, vp, vp, vp, i]
        lib.ocvar_hip_find_squares.argtypes = [vp, vp, i, i, i, vp, i, vp]
        lib.ocvar_hip_debug_gray.argtypes = [vp, i, vp]
        lib.ocvar_hip_debug_binary.argtypes = [vp, i, vp]
        lib.ocvar_hip_debug_masks.argtypes = [vp, i, vp]
        lib.ocvar_hip_debug_frame_quads.argtypes = [vp, i, vp, vp]
        lib.ocvar_hip_debug_candidates.argtypes = [vp, i, vp, i, vp]
        lib.ocvar_hip_debug_crop_rois.argtypes = [vp, vp, i, vp]
        lib.ocvar_hip_debug_crop_plane.argtypes = [vp, i, i, vp]
        lib.ocvar_hip_debug_starts.argtypes = [vp, i, vp, i, vp]
        lib.ocvar_hip_debug_rings.argtypes = [vp, i, vp, i, vp]
        lib.ocvar_hip_stage_ms.argtypes = [vp, vp, i]
        lib.ocvar_hip_counters.argtypes = [vp, vp, i]
        lib.ocvar_hip_stage_stamps.argtypes = [vp, vp, vp, i]
        lib.ocvar_hip_stream.argtypes = [vp]
        lib.ocvar_hip_stream.restype = vp
        lib.ocvar_hip_results_to_device.argtypes = [vp, vp, vp, vp]
        lib.ocvar_hip_results_to_device_ex.argtypes = [vp, vp, vp, i, vp]
        lib.ocvar_hip_debug_calibrate.argtypes = [vp, sz]
        lib.ocvar_hip_set_board.argtypes = [vp, vp, i]
        lib.ocvar_hip_board_poses.argtypes = [vp, vp, i]
        lib.ocvar_hip_board_poses_to_device.argtypes = [vp, vp, vp]
        lib.ocvar_hip_set_overlay.argtypes = [vp, i, vp, i, i, i]
        lib.ocvar_hip_render.argtypes = [vp, vp, i, i, i, sz, i, vp]
        lib.ocvar_hip_render_records.argtypes = [vp, vp, i, i, i, sz, i, i, vp, vp, i, vp]
        lib.ocvar_hip_annotate_default_style.argtypes = [vp]
        lib.ocvar_hip_annotate.argtypes = [vp, vp, i, i, i, sz, i, vp, vp]
        lib.ocvar_hip_annotate_records.argtypes = [vp, vp, i, i, i, sz, i, i, vp, vp, i, vp, vp]
        lib.ocvar_hip_patches.argtypes = [vp, vp, i, i, i, sz, i, vp, i, i, i, i, vp, vp]
        lib.ocvar_hip_patches_records.argtypes = [vp, vp, i, i, i, sz, i, i, vp, vp, i, vp, i, i, i, vp, vp]
        lib.ocvar_hip_undistort.argtypes = [vp, vp, i, sz, vp, i, sz, i, i, i, i, vp]
        lib.ocvar_hip_undistort_records.argtypes = [vp, vp, vp, i, i, vp, vp]
        lib.ocvar_hip_flow_records.argtypes = [vp, vp, i, sz, vp, i, sz, i, i, i, i, vp, vp, i, vp, vp, vp, vp, vp]
        lib.ocvar_hip_yuv_to_frames.argtypes = [vp, vp, vp, i, sz, i, i, i, i, vp]
        lib.ocvar_hip_frames_to_yuv.argtypes = [vp, vp, i, sz, vp, i, i, i, i, vp]
        lib.ocvar_hip_yuv_to_frames_ex.argtypes = [vp, vp, vp, i, sz, i, i, i, i, vp]
        lib.ocvar_hip_frames_to_yuv_ex.argtypes = [vp, vp, i, sz, vp, i, i, i, i, vp]
        lib.ocvar_hip_resize.argtypes = [vp, vp, i, i, i, sz, vp, i, i, i, sz, i, i, i, vp]
        lib.ocvar_hip_scale_records.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, vp, vp]
        lib.ocvar_hip_orient.argtypes = [vp, vp, i, i, i, sz, vp, i, sz, i, i, i, vp]
        lib.ocvar_hip_orient_records.argtypes = [vp, vp, vp, i, i, i, i, i, i, vp, vp]
        lib.ocvar_hip_orient_camera.argtypes = [vp, i, vp]
        lib.ocvar_hip_warp.argtypes = [vp, vp, i, i, i, sz, vp, i, i, i, sz, i, i, vp, i, i, vp, i, vp, vp]
        lib.ocvar_hip_warp_records.argtypes = [vp, vp, vp, i, i, vp, i, vp, vp]
        lib.ocvar_hip_board_plane_maps.argtypes = [vp, vp, i, vp, i, i, vp, vp]
        lib.ocvar_hip_levels_default_params.argtypes = [vp]
        lib.ocvar_hip_levels.argtypes = [vp, vp, i, i, i, sz, i, vp, i, sz, i, vp, vp]
        lib.ocvar_hip_bayer_default_params.argtypes = [vp]
        lib.ocvar_hip_bayer_pattern_at.argtypes = [i, i, i]
        lib.ocvar_hip_bayer_to_frames.argtypes = [vp, vp, i, sz, vp, i, sz, i, i, i, i, vp, vp]
        _hip = lib
    return _hip


_host = None


def host_lib():
    """The host C++ mirror of the reference's public API (libopencv-ar.so: cvarLoadTemplateTag, cvarReadCamera, ...)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise OcvarError(f"{HOST_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        hip_lib()   # libopencv-ar.so links against the HIP library: same runtime-ordering rule
        lib = C.CDLL(HOST_LIB)
        lib.cvarLoadTemplateTag.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        lib.cvarReadCamera.argtypes = [C.c_char_p, C.c_void_p]
        lib.cvarCameraScale.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _host = lib
    return _host


TEMPLATE_DIR = os.path.join(os.path.dirname(_HERE), "assets", "templates")


def orient_camera(camera, o):
    """the Camera of the frames orientation o makes from the frames of `camera` (a new Camera): width and height of the turned
    frames, fx and fy swapped when o transposes, the principal point carried like a pixel, the tangential distortion pair turned
    with the image plane, glProjection computed as cvarCameraScale does.  ValueError for a camera matrix with skew (or one that is
    not fx 0 cx / 0 fy cy / 0 0 1) under any orientation but 'identity'."""
    out = Camera()
    if hip_lib().ocvar_hip_orient_camera(C.byref(camera), orientation_code(o), C.byref(out)) != 0:
        raise ValueError("orient_camera: the camera matrix must be fx 0 cx / 0 fy cy / 0 0 1")
    return out


def load_templates(paths, scale=0.01):
    """cvarLoadTemplateTag (reference opencvar.cpp:284-321) on each PNG -> list of Template."""
    out = []
    for path in paths:
        t = Template()
        if host_lib().cvarLoadTemplateTag(C.byref(t), os.fsencode(path), scale) != 1:
            raise OcvarError(f"cvarLoadTemplateTag failed for {path}")
        out.append(t)
    return out


def default_camera(width, height, filename=None):
    """cvarReadCamera(filename or NULL) then cvarCameraScale(width, height) (opencvar.cpp:37-102)."""
    cam = Camera()
    if host_lib().cvarReadCamera(os.fsencode(filename) if filename else None, C.byref(cam)) != 1:
        raise OcvarError(f"cvarReadCamera failed for {filename}")
    host_lib().cvarCameraScale(C.byref(cam), width, height)
    return cam


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class Gate:
    """At most `width` binarise kernels of the detectors that share the gate run at once, and their batches are placed on the
    gate's `lanes` streams (0: one per hardware queue of the process; include/ocvar_hip.h)."""

    def __init__(self, width=2, device=0, lanes=0):
        self._lib = hip_lib()
        self._g = C.c_void_p()
        rc = self._lib.ocvar_hip_gate_create_lanes(C.byref(self._g), device, width, lanes)
        if rc != 0:
            raise OcvarError(f"ocvar_hip_gate_create_lanes failed ({rc})")

    @property
    def lanes(self):
        return self._lib.ocvar_hip_gate_lanes(self._g)

    def __del__(self):
        if getattr(self, "_g", None):
            self._lib.ocvar_hip_gate_destroy(self._g)
            self._g = None


class Pipe:
    """Several contexts on one GPU as one detector (include/ocvar_hip.h: ocvar_hip_pipe_*): device-resident frames, any number
    of them, detected chunk by chunk with one chunk in flight per context."""

    input_format = INPUT_FORMATS["bgr"]   # (set_input_format)

    def __init__(self, max_width, max_height, chunk_frames=2048, n_contexts=4, gate_width=2, device=0):
        self._lib = hip_lib()
        self._p = C.c_void_p()
        self.chunk_frames = chunk_frames
        rc = self._lib.ocvar_hip_pipe_create(C.byref(self._p), device, max_width, max_height, chunk_frames, n_contexts, gate_width)
        if rc != 0:
            msg = self._lib.ocvar_hip_pipe_last_error(self._p).decode() if self._p else ""
            self.close()
            raise OcvarError(f"ocvar_hip_pipe_create failed ({rc}): {msg}")

    def close(self):
        if getattr(self, "_p", None):
            self._lib.ocvar_hip_pipe_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: module globals may be gone
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise OcvarError(f"{what} failed ({rc}): {self._lib.ocvar_hip_pipe_last_error(self._p).decode()}")

    def set_templates(self, templates):
        arr = (Template * len(templates))(*templates)
        self._check(self._lib.ocvar_hip_pipe_set_templates(self._p, arr, len(templates)), "pipe_set_templates")

    def set_camera(self, camera):
        self._check(self._lib.ocvar_hip_pipe_set_camera(self._p, C.byref(camera)), "pipe_set_camera")

    def set_input_format(self, fmt):
        """what the frames of detect_device / submit / track_device hold: 'bgr' (default), 'rgb', 'bgra', 'rgba' or 'gray'"""
        code = input_format_code(fmt)
        self._check(self._lib.ocvar_hip_pipe_set_input_format(self._p, code), "pipe_set_input_format")
        self.input_format = code

    def set_corner_refine(self, half_win=5, max_iter=30, eps=0.1):
        """sub-pixel corner refinement of every context (Detector.set_corner_refine); half_win=0 turns it off.  OcvarError while a
        submitted chunk is in flight"""
        w, it, e = corner_refine_args(half_win, max_iter, eps)
        self._check(self._lib.ocvar_hip_pipe_set_corner_refine(self._p, w, it, e), "pipe_set_corner_refine")

    def detect_device(self, d_ptr, width, height, n_frames, row_stride=None, frame_stride=None, grey_in_place=False, max_per_frame=MAX_MARKERS):
        row_stride = row_stride or FORMAT_BPP[self.input_format] * width
        frame_stride = frame_stride or row_stride * height
        markers = np.zeros((n_frames, max_per_frame), MARKER_DTYPE)
        counts = np.zeros(n_frames, np.int32)
        self._check(self._lib.ocvar_hip_pipe_detect_device(self._p, d_ptr, width, height, row_stride, frame_stride, n_frames,
                                                           int(grey_in_place), _ptr(markers), _ptr(counts), max_per_frame), "pipe_detect_device")
        return markers, counts

    def submit(self, d_ptr, width, height, n_frames, tag=0, row_stride=None, frame_stride=None, grey_in_place=False):
        """streaming form: hand the next chunk to the next context; False when every context already has one in flight"""
        row_stride = row_stride or FORMAT_BPP[self.input_format] * width
        frame_stride = frame_stride or row_stride * height
        rc = self._lib.ocvar_hip_pipe_submit(self._p, d_ptr, width, height, row_stride, frame_stride, n_frames, int(grey_in_place), tag)
        if rc == -6:
            return False
        self._check(rc, "pipe_submit")
        return True

    def collect(self, max_frames, max_per_frame=MAX_MARKERS):
        """the oldest chunk in flight: (tag, markers [n][max_per_frame], counts [n]) or None when nothing is in flight.
        max_per_frame must not exceed the pipe's result limit (set_result_limit)."""
        # the C call writes one row per frame of the chunk, up to chunk_frames of them, whatever max_frames says
        rows = max(max_frames, self.chunk_frames)
        markers = np.zeros((rows, max_per_frame), MARKER_DTYPE)
        counts = np.zeros(rows, np.int32)
        tag = C.c_longlong(0)
        n = self._lib.ocvar_hip_pipe_collect(self._p, C.byref(tag), _ptr(markers), _ptr(counts), max_per_frame)
        if n < 0:
            self._check(n, "pipe_collect")
        if n == 0:
            return None
        return tag.value, markers[:n], counts[:n]

    def in_flight(self):
        return self._lib.ocvar_hip_pipe_in_flight(self._p)

    def set_result_limit(self, max_per_frame):
        self._check(self._lib.ocvar_hip_pipe_set_result_limit(self._p, max_per_frame), "pipe_set_result_limit")

    def track_device(self, d_ptr, width, height, n_streams, reset=False, row_stride=None, frame_stride=None, grey_in_place=False,
                     max_per_frame=MAX_MARKERS):
        """one time step of n_streams video streams (frame s = stream s); the streams' markers of the previous step stay on the device"""
        row_stride = row_stride or FORMAT_BPP[self.input_format] * width
        frame_stride = frame_stride or row_stride * height
        markers = np.zeros((n_streams, max_per_frame), MARKER_DTYPE)
        counts = np.zeros(n_streams, np.int32)
        self._check(self._lib.ocvar_hip_pipe_track_device(self._p, d_ptr, width, height, row_stride, frame_stride, n_streams,
                                                          int(grey_in_place), int(reset), _ptr(markers), _ptr(counts), max_per_frame), "pipe_track_device")
        return markers, counts


def build_info():
    """how libocvar_hip.so was built (flags that change what the kernels do: profiling hooks, tuning switches)"""
    return hip_lib().ocvar_hip_build_info().decode()


class Detector:
    """A device context: batches of frames -> CvarMarker arrays (cvarArMultRegistration semantics per frame).

    max_quads / max_markers (either one): a dense context (ocvar_hip_create_dense) with room for that many frame-pass squares
    (1 .. MAX_QUADS_DENSE, default MAX_QUADS) and markers (1 .. MAX_MARKERS_DENSE, default MAX_MARKERS) per frame.  Result
    arrays and `prev` blocks are [n, det.max_markers]."""

    input_format = INPUT_FORMATS["bgr"]   # what the frames hold (set_input_format)
    max_markers = MAX_MARKERS             # the context's marker stride M (ocvar_hip_max_markers)
    max_quads = MAX_QUADS                 # squares per frame find_squares / debug_frame_quads bring back

    def __init__(self, max_width, max_height, max_batch=1, device=0, max_quads=None, max_markers=None):
        self._lib = hip_lib()
        self._ctx = C.c_void_p()
        dense = max_quads is not None or max_markers is not None
        if dense:
            q = MAX_QUADS if max_quads is None else int(max_quads)
            m = MAX_MARKERS if max_markers is None else int(max_markers)
            rc = self._lib.ocvar_hip_create_dense(C.byref(self._ctx), device, max_width, max_height, max_batch, q, m)
        else:
            rc = self._lib.ocvar_hip_create(C.byref(self._ctx), device, max_width, max_height, max_batch)
        if rc != 0:
            msg = self._lib.ocvar_hip_last_error(self._ctx).decode() if self._ctx else "no gfx950 device or bad arguments"
            if self._ctx:
                self._lib.ocvar_hip_destroy(self._ctx)
                self._ctx = C.c_void_p()
            raise OcvarError(f"{'ocvar_hip_create_dense' if dense else 'ocvar_hip_create'} failed ({rc}): {msg}")
        if dense:
            self.max_quads = q
            self.max_markers = self._lib.ocvar_hip_max_markers(self._ctx)
        self.max_batch = max_batch
        self.n_templates = 0

    def close(self):
        if self._ctx:
            self._lib.ocvar_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise OcvarError(f"{what} failed ({rc}): {self._lib.ocvar_hip_last_error(self._ctx).decode()}")

    def set_templates(self, templates):
        arr = (Template * len(templates))(*templates)
        self._check(self._lib.ocvar_hip_set_templates(self._ctx, arr, len(templates)), "set_templates")
        self.n_templates = len(templates)

    def set_camera(self, camera):
        self._check(self._lib.ocvar_hip_set_camera(self._ctx, C.byref(camera)), "set_camera")

    def _prev_arrays(self, prev, n_frames):
        if prev is None:
            return None, None
        M = self.max_markers
        pm = np.zeros((n_frames, M), MARKER_DTYPE)
        pc = np.zeros(n_frames, np.int32)
        for f, lst in enumerate(prev):
            pc[f] = min(len(lst), M)
            for k in range(pc[f]):
                pm[f, k] = lst[k]
        return pm, pc

    def _strides(self, fmt, width, height, row_stride, frame_stride, bpp=None):
        """(format code, row stride, frame stride) of frames of width x height pixels in fmt (None: the input format): a stride
        that is not given is that of packed rows or frames; bpp: the bytes per pixel where they are not the format's"""
        code = self.input_format if fmt is None else input_format_code(fmt)
        row_stride = row_stride or (bpp or FORMAT_BPP[code]) * width
        return code, row_stride, frame_stride or row_stride * height

    def enqueue_device(self, d_ptr, width, height, n_frames, row_stride=None, frame_stride=None, grey_in_place=False,
                       prev=None, stream=None):
        _, row_stride, frame_stride = self._strides(None, width, height, row_stride, frame_stride)
        pm, pc = self._prev_arrays(prev, n_frames)
        self._keep = (pm, pc)
        self._check(self._lib.ocvar_hip_enqueue(self._ctx, d_ptr, width, height, row_stride, frame_stride, n_frames,
                                                int(grey_in_place), _ptr(pm), _ptr(pc), stream), "enqueue")
        self._n = n_frames

    def enqueue_tracked(self, d_ptr, width, height, n_frames, d_prev_ptr, d_prev_counts_ptr, row_stride=None, frame_stride=None,
                        grey_in_place=False, stream=None):
        """enqueue with the previous markers in device memory: d_prev [n_frames, max_markers] records, d_prev_counts [n_frames]
        (ocvar_hip_enqueue_tracked); collect() as after enqueue_device"""
        _, row_stride, frame_stride = self._strides(None, width, height, row_stride, frame_stride)
        self._check(self._lib.ocvar_hip_enqueue_tracked(self._ctx, d_ptr, width, height, row_stride, frame_stride, n_frames,
                                                        int(grey_in_place), d_prev_ptr, d_prev_counts_ptr, stream), "enqueue_tracked")
        self._n = n_frames

    def collect(self, max_per_frame=None):
        max_per_frame = self.max_markers if max_per_frame is None else max_per_frame
        n = self._n
        markers = np.zeros((n, max_per_frame), MARKER_DTYPE)
        counts = np.zeros(n, np.int32)
        self._check(self._lib.ocvar_hip_collect(self._ctx, _ptr(markers), _ptr(counts), max_per_frame), "collect")
        return markers, counts

    def ready(self):
        """True once the enqueued batch has finished (collect() will not wait)"""
        rc = self._lib.ocvar_hip_ready(self._ctx)
        if rc < 0:
            self._check(rc, "ready")
        return rc == 1

    def set_result_limit(self, max_per_frame):
        """marker records per frame a batch brings to the host (1 .. max_markers, the default); counts stay the full counts"""
        self._check(self._lib.ocvar_hip_set_result_limit(self._ctx, max_per_frame), "set_result_limit")

    def set_input_format(self, fmt):
        """what the frames of later batches hold: 'bgr' (default), 'rgb', 'bgra', 'rgba' or 'gray' (include/ocvar_hip.h:
        the results are the reference's on the BGR frame of the same colours)"""
        code = input_format_code(fmt)
        self._check(self._lib.ocvar_hip_set_input_format(self._ctx, code), "set_input_format")
        self.input_format = code

    def set_corner_refine(self, half_win=5, max_iter=30, eps=0.1):
        """sub-pixel refinement of the output markers' corners on the grey frame (OpenCV's cornerSubPix equations:
        include/ocvar_hip.h, ocvar_hip_set_corner_refine), and poses solved from the refined corners, from the next batch on.
        half_win 0 (the default of a new detector) turns it off; 5 / 30 / 0.1 is ArUco's typical setting."""
        w, it, e = corner_refine_args(half_win, max_iter, eps)
        self._check(self._lib.ocvar_hip_set_corner_refine(self._ctx, w, it, e), "set_corner_refine")

    def set_board(self, entries):
        """A planar marker board, from the next batch on: entries = [(template_id, 4x2 board-plane corners)] (grid_board makes
        them; corners 0..3 as include/ocvar_hip.h defines them), up to MAX_BOARD_MARKERS; None or [] turns it off (the default).
        Every collected batch then has one pose per frame: board_poses()."""
        entries = [] if entries is None else list(entries)
        arr = (BoardMarker * max(len(entries), 1))()
        for k, (t, corners) in enumerate(entries):
            c = np.asarray(corners, np.float64)
            if c.shape != (4, 2):
                raise ValueError(f"board entry {k}: corners must be 4 x 2, got {c.shape}")
            arr[k].templateId = int(t)
            arr[k].corner[:] = c.reshape(8).tolist()
        self._check(self._lib.ocvar_hip_set_board(self._ctx, arr, len(entries)), "set_board")

    def board_poses(self):
        """[n] BOARD_DTYPE: the board pose of every frame of the last collected batch (all frames of a detect_host call)"""
        out = np.zeros(self._n, BOARD_DTYPE)
        self._check(self._lib.ocvar_hip_board_poses(self._ctx, _ptr(out), self._n), "board_poses")
        return out

    def board_poses_to_device(self, d_poses_ptr, stream=None):
        """after enqueue: stream-ordered copy of the batch's [n] board poses (192 bytes each) into caller-owned device memory"""
        self._check(self._lib.ocvar_hip_board_poses_to_device(self._ctx, d_poses_ptr, stream), "board_poses_to_device")

    def set_overlay(self, template_id, rgba):
        """The overlay image drawn on every marker of template template_id (-1: the default overlay, for every template without
        one of its own): an H x W x 4 uint8 array, straight-alpha R G B A, 2 .. MAX_OVERLAY_SIDE texels each way; None removes it.
        Row 0 of the array lands along the edge between record corners 0 and 1 (include/ocvar_hip.h says which way up that is).
        At most MAX_OVERLAYS per detector.  OcvarError while a batch is in flight."""
        if rgba is None:
            self._check(self._lib.ocvar_hip_set_overlay(self._ctx, int(template_id), None, 0, 0, 0), "set_overlay")
            return
        a = np.asarray(rgba)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
            raise ValueError(f"an overlay is an H x W x 4 uint8 array, got {a.dtype} {a.shape}")
        a = np.ascontiguousarray(a)
        self._check(self._lib.ocvar_hip_set_overlay(self._ctx, int(template_id), _ptr(a), a.shape[1], a.shape[0], 4 * a.shape[1]), "set_overlay")

    def render(self, d_ptr, width, height, fmt=None, row_stride=None, frame_stride=None, stream=None):
        """between enqueue and collect: draws the overlays onto the enqueued batch's markers in the device frames at d_ptr (the
        frames detected, or another buffer of the batch's frame count and size) in format fmt (default: the input format);
        stream-ordered behind the batch, does not wait"""
        code, row_stride, frame_stride = self._strides(fmt, width, height, row_stride, frame_stride)
        self._check(self._lib.ocvar_hip_render(self._ctx, d_ptr, width, height, row_stride, frame_stride, code, stream), "render")

    def render_records(self, d_ptr, width, height, n_frames, d_markers_ptr, d_counts_ptr, per_frame=None, fmt=None, row_stride=None,
                       frame_stride=None, stream=None):
        """draws the overlays onto n_frames device frames under caller-supplied device records [n_frames, per_frame] (default
        per_frame: max_markers) and counts [n_frames]; needs no batch, does not wait (stream None: the detector's own stream)"""
        per_frame = self.max_markers if per_frame is None else per_frame
        code, row_stride, frame_stride = self._strides(fmt, width, height, row_stride, frame_stride)
        self._check(self._lib.ocvar_hip_render_records(self._ctx, d_ptr, width, height, row_stride, frame_stride, n_frames, code,
                                                       d_markers_ptr, d_counts_ptr, per_frame, stream), "render_records")

    def annotate(self, d_ptr, width, height, style=None, fmt=None, row_stride=None, frame_stride=None, stream=None):
        """between enqueue and collect: strokes outlines, corner-0 dots, pose axes and cubes and template ids (what `style`, an
        annotate_style(), asks for; default: the library's default style) of the enqueued batch's markers into the device frames
        at d_ptr (the frames detected, or another buffer of the batch's frame count and size) in format fmt (default: the input
        format); stream-ordered behind the batch -- and behind a render called before it -- does not wait"""
        code, row_stride, frame_stride = self._strides(fmt, width, height, row_stride, frame_stride)
        st = annotate_style() if style is None else AnnotateStyle.from_buffer_copy(bytes(style))
        self._check(self._lib.ocvar_hip_annotate(self._ctx, d_ptr, width, height, row_stride, frame_stride, code, C.byref(st), stream), "annotate")

    def annotate_records(self, d_ptr, width, height, n_frames, d_markers_ptr, d_counts_ptr, per_frame=None, style=None, fmt=None,
                         row_stride=None, frame_stride=None, stream=None):
        """the same on n_frames device frames under caller-supplied device records [n_frames, per_frame] (default per_frame:
        max_markers) and counts [n_frames]; needs no batch, does not wait (stream None: the detector's own stream)"""
        per_frame = self.max_markers if per_frame is None else per_frame
        code, row_stride, frame_stride = self._strides(fmt, width, height, row_stride, frame_stride)
        st = annotate_style() if style is None else AnnotateStyle.from_buffer_copy(bytes(style))
        self._check(self._lib.ocvar_hip_annotate_records(self._ctx, d_ptr, width, height, row_stride, frame_stride, n_frames, code,
                                                         d_markers_ptr, d_counts_ptr, per_frame, C.byref(st), stream), "annotate_records")

    def patches(self, d_ptr, width, height, d_patches_ptr, patch_w, patch_h, per_frame=None, fmt=None, row_stride=None, frame_stride=None,
                flip_rows=False, matched_only=False, d_status_ptr=None, stream=None):
        """between enqueue and collect: the rectified patch_h x patch_w image of the first per_frame (default max_markers) records
        of every frame of the enqueued batch, cut out of the device frames at d_ptr (the frames detected, or another buffer of the
        batch's frame count and size) in format fmt (default: the input format), into the device block d_patches_ptr
        [n, per_frame, patch_h, patch_w, bpp] uint8; record corners 0..3 land on the patch's top-left, top-right, bottom-right and
        bottom-left pixels (flip_rows: rows stored bottom-up, as the template's image file reads).  d_status_ptr: device ints
        [n, per_frame], 1 where the slot was written; slots that are not written keep their bytes (include/ocvar_hip.h has the
        rule).  matched_only: records with score > 0 only.  Stream-ordered behind the batch, does not wait."""
        per_frame = self.max_markers if per_frame is None else per_frame
        code, row_stride, frame_stride = self._strides(fmt, width, height, row_stride, frame_stride)
        flags = (PATCH_FLIP_ROWS if flip_rows else 0) | (PATCH_MATCHED_ONLY if matched_only else 0)
        self._check(self._lib.ocvar_hip_patches(self._ctx, d_ptr, width, height, row_stride, frame_stride, code, d_patches_ptr, patch_w,
                                                patch_h, per_frame, flags, d_status_ptr, stream), "patches")

    def patches_records(self, d_ptr, width, height, n_frames, d_markers_ptr, d_counts_ptr, d_patches_ptr, patch_w, patch_h, per_frame=None,
                        fmt=None, row_stride=None, frame_stride=None, flip_rows=False, matched_only=False, d_status_ptr=None, stream=None):
        """the same for n_frames device frames under caller-supplied device records [n_frames, per_frame] (default per_frame:
        max_markers) and counts [n_frames]; needs no batch, does not wait (stream None: the detector's own stream)"""
        per_frame = self.max_markers if per_frame is None else per_frame
        code, row_stride, frame_stride = self._strides(fmt, width, height, row_stride, frame_stride)
        flags = (PATCH_FLIP_ROWS if flip_rows else 0) | (PATCH_MATCHED_ONLY if matched_only else 0)
        self._check(self._lib.ocvar_hip_patches_records(self._ctx, d_ptr, width, height, row_stride, frame_stride, n_frames, code,
                                                        d_markers_ptr, d_counts_ptr, per_frame, d_patches_ptr, patch_w, patch_h, flags,
                                                        d_status_ptr, stream), "patches_records")

    def undistort(self, d_src, d_dst, width, height, n_frames, fmt=None, src_row_stride=None, src_frame_stride=None, dst_row_stride=None,
                  dst_frame_stride=None, stream=None):
        """n_frames device frames at d_src in format fmt (default: the input format), taken with the camera of set_camera, into the
        device frames at d_dst as a pinhole camera with the same camera matrix sees them (OpenCV's undistort with newCameraMatrix =
        cameraMatrix; 0 where the source lies outside the frame).  Source and destination must not overlap.  Needs no batch, does
        not wait (stream None: the detector's own stream); the camera is the one set at the call."""
        code, src_row_stride, src_frame_stride = self._strides(fmt, width, height, src_row_stride, src_frame_stride)
        code, dst_row_stride, dst_frame_stride = self._strides(fmt, width, height, dst_row_stride, dst_frame_stride)
        self._check(self._lib.ocvar_hip_undistort(self._ctx, d_src, src_row_stride, src_frame_stride, d_dst, dst_row_stride, dst_frame_stride,
                                                  width, height, n_frames, code, stream), "undistort")

    def undistort_records(self, d_markers, d_counts, n_frames, d_out, per_frame=None, stream=None):
        """the squares of the device records [n_frames, per_frame] (default per_frame: max_markers) under counts [n_frames] moved
        to where the undistorted frames show them (OpenCV's undistortPoints with P = cameraMatrix), every other field copied, into
        the device records at d_out (which may be d_markers); slots at or beyond a frame's count are not written.  Needs no
        batch, does not wait (stream None: the detector's own stream)."""
        per_frame = self.max_markers if per_frame is None else per_frame
        self._check(self._lib.ocvar_hip_undistort_records(self._ctx, d_markers, d_counts, n_frames, per_frame, d_out, stream),
                    "undistort_records")

    @staticmethod
    def _yuv_call(yuv, plain, ex):
        """the entry point that takes the descriptor: a YuvFrames goes to the 8-bit limited-range call, a YuvFramesEx to the _ex one"""
        if isinstance(yuv, YuvFramesEx):
            return ex
        if isinstance(yuv, YuvFrames):
            return plain
        raise TypeError(f"a YuvFrames or a YuvFramesEx describes the YUV frames, got {type(yuv).__name__}")

    def yuv_to_frames(self, yuv, d_dst, width, height, n_frames, fmt=None, dst_row_stride=None, dst_frame_stride=None, stream=None):
        """n_frames device frames in NV12, I420, YUYV or UYVY (yuv: a YuvFrames) converted into the device frames at d_dst in format
        fmt (default: the input format): OpenCV's cvtColor COLOR_YUV2BGR_NV12 and its relatives, limited range, the matrix yuv names.
        A four-channel destination gets byte 3 = 255, 'gray' the library's grey of the converted colour.  The two sides must not
        overlap.  Needs no batch, does not wait (stream None: the detector's own stream).  With a YuvFramesEx: any of its layouts
        ('nv21', 'i444' too), ranges, matrices and depths (P010, P012, P016), through ocvar_hip_yuv_to_frames_ex."""
        code, dst_row_stride, dst_frame_stride = self._strides(fmt, width, height, dst_row_stride, dst_frame_stride)
        call = self._yuv_call(yuv, self._lib.ocvar_hip_yuv_to_frames, self._lib.ocvar_hip_yuv_to_frames_ex)
        self._check(call(self._ctx, C.byref(yuv), d_dst, dst_row_stride, dst_frame_stride, width, height, n_frames, code, stream), "yuv_to_frames")

    def frames_to_yuv(self, d_src, yuv, width, height, n_frames, fmt=None, src_row_stride=None, src_frame_stride=None, stream=None):
        """n_frames device frames at d_src in format fmt (default: the input format) converted into the NV12, I420, YUYV or UYVY device
        frames yuv (a YuvFrames) describes: OpenCV's cvtColor COLOR_BGR2YUV_I420 and its relatives, limited range, a chroma sample from
        the mean colour of its 2 x 2 or 2 x 1 pixels.  The two sides must not overlap.  Needs no batch, does not wait (stream None:
        the detector's own stream).  With a YuvFramesEx: any of its layouts, ranges, matrices and depths, a 4:4:4 chroma sample from
        its own pixel, the low bits of a 16-bit word zero, through ocvar_hip_frames_to_yuv_ex."""
        code, src_row_stride, src_frame_stride = self._strides(fmt, width, height, src_row_stride, src_frame_stride)
        call = self._yuv_call(yuv, self._lib.ocvar_hip_frames_to_yuv, self._lib.ocvar_hip_frames_to_yuv_ex)
        self._check(call(self._ctx, d_src, src_row_stride, src_frame_stride, C.byref(yuv), width, height, n_frames, code, stream), "frames_to_yuv")

    def resize(self, d_src, src_width, src_height, d_dst, dst_width, dst_height, n_frames, interp="area", fmt=None, src_row_stride=None,
               src_frame_stride=None, dst_row_stride=None, dst_frame_stride=None, stream=None):
        """n_frames device frames of src_width x src_height pixels at d_src in format fmt (default: the input format) resized into
        the device frames of dst_width x dst_height at d_dst: OpenCV's resize on 8-bit images with interp 'nearest', 'linear' or
        'area' ('area' shrinks only, by at most 16 per axis; a whole-number ratio is the rounded mean of the block).  The sizes are
        not bound by the detector's: large frames feed a small detector.  A source rectangle is d_src moved to its first pixel with
        the full frame's strides.  Source and destination must not overlap.  Needs no batch, does not wait (stream None: the
        detector's own stream)."""
        if not (isinstance(interp, str) and interp.lower() in RESIZE_INTERPS):
            raise ValueError(f"unknown interpolation {interp!r}: one of {sorted(RESIZE_INTERPS)}")
        code, src_row_stride, src_frame_stride = self._strides(fmt, src_width, src_height, src_row_stride, src_frame_stride)
        code, dst_row_stride, dst_frame_stride = self._strides(fmt, dst_width, dst_height, dst_row_stride, dst_frame_stride)
        self._check(self._lib.ocvar_hip_resize(self._ctx, d_src, src_width, src_height, src_row_stride, src_frame_stride, d_dst, dst_width,
                                               dst_height, dst_row_stride, dst_frame_stride, n_frames, code, RESIZE_INTERPS[interp.lower()],
                                               stream), "resize")

    def scale_records(self, d_markers, d_counts, n_frames, d_out, src_size, dst_size, per_frame=None, pose=False, stream=None):
        """the squares of the device records [n_frames, per_frame] (default per_frame: max_markers) under counts [n_frames], found on
        frames of src_size = (width, height), carried to frames of dst_size by the pixel-centre rule of resize, every other field
        copied, into the device records at d_out (which may be d_markers); slots at or beyond a frame's count are not written.
        pose: glMatrix is solved again from the new square with the camera set at the call, which must be that of dst_size.  Needs no
        batch, does not wait (stream None: the detector's own stream)."""
        per_frame = self.max_markers if per_frame is None else per_frame
        self._check(self._lib.ocvar_hip_scale_records(self._ctx, d_markers, d_counts, n_frames, per_frame, src_size[0], src_size[1],
                                                      dst_size[0], dst_size[1], SCALE_POSE if pose else 0, d_out, stream), "scale_records")

    def orient(self, d_src, src_width, src_height, d_dst, n_frames, orientation, fmt=None, src_row_stride=None, src_frame_stride=None,
               dst_row_stride=None, dst_frame_stride=None, stream=None):
        """n_frames device frames of src_width x src_height pixels at d_src in format fmt (default: the input format) turned or
        mirrored into the device frames at d_dst, whose size is oriented_size((src_width, src_height), orientation): OpenCV's rotate,
        flip and transpose, a pure permutation of pixels.  orientation: a name of ORIENTATIONS ('rot90' is clockwise) or its code.
        The sizes are not bound by the detector's.  A source rectangle is d_src moved to its first pixel with the full frame's
        strides.  Source and destination must not overlap, 'identity' included.  Needs no batch, does not wait (stream None: the
        detector's own stream)."""
        o = orientation_code(orientation)
        dst_width, dst_height = oriented_size((src_width, src_height), o)
        code, src_row_stride, src_frame_stride = self._strides(fmt, src_width, src_height, src_row_stride, src_frame_stride)
        code, dst_row_stride, dst_frame_stride = self._strides(fmt, dst_width, dst_height, dst_row_stride, dst_frame_stride)
        self._check(self._lib.ocvar_hip_orient(self._ctx, d_src, src_width, src_height, src_row_stride, src_frame_stride, d_dst, dst_row_stride,
                                               dst_frame_stride, n_frames, code, o, stream), "orient")

    def orient_records(self, d_markers, d_counts, n_frames, d_out, src_size, orientation, per_frame=None, pose=False, stream=None):
        """the squares of the device records [n_frames, per_frame] (default per_frame: max_markers) under counts [n_frames], found on
        frames of src_size = (width, height), carried to where orient(..., orientation) puts those frames' pixels, every other field
        copied, into the device records at d_out (which may be d_markers); slots at or beyond a frame's count are not written.
        Corner k stays in slot k: the mirroring orientations reverse the winding of the square.  pose: glMatrix is solved again from
        the new square with the camera set at the call, which must be orient_camera(camera of src_size, orientation); refused for
        the mirroring orientations.  Needs no batch, does not wait (stream None: the detector's own stream)."""
        per_frame = self.max_markers if per_frame is None else per_frame
        self._check(self._lib.ocvar_hip_orient_records(self._ctx, d_markers, d_counts, n_frames, per_frame, src_size[0], src_size[1],
                                                       orientation_code(orientation), ORIENT_POSE if pose else 0, d_out, stream), "orient_records")

    def levels(self, d_src, d_dst, width, height, n_frames, params=None, fmt=None, src_row_stride=None, src_frame_stride=None,
               dst_row_stride=None, dst_frame_stride=None, stream=None):
        """n_frames device frames of width x height pixels at d_src in format fmt (default: the input format) with their grey levels
        stretched into one GRAY plane per frame at d_dst: per tile of params' grid the grey values between the clipped ends of the
        tile's histogram are spread over 0 .. 255 (the gain capped), and a pixel takes the blend of the maps of the four tiles
        around it (params: levels_params(...); None: one map per frame, 1 % clipped at each end, a gain of at most 8).  Detected
        with set_input_format('gray') the planes yield records in the source frames' own coordinates.  The sizes are not bound by
        the detector's.  Source and destination must not overlap.  The first call allocates a workspace of 20 MiB.  Needs no batch,
        does not wait (stream None: the detector's own stream)."""
        code, src_row_stride, src_frame_stride = self._strides(fmt, width, height, src_row_stride, src_frame_stride)
        _, dst_row_stride, dst_frame_stride = self._strides(fmt, width, height, dst_row_stride, dst_frame_stride, bpp=1)   # (GRAY)
        self._check(self._lib.ocvar_hip_levels(self._ctx, d_src, width, height, src_row_stride, src_frame_stride, code, d_dst, dst_row_stride,
                                               dst_frame_stride, n_frames, None if params is None else C.byref(params), stream), "levels")

    def bayer_to_frames(self, d_src, d_dst, width, height, n_frames, params=None, fmt=None, src_row_stride=None, src_frame_stride=None,
                        dst_row_stride=None, dst_frame_stride=None, stream=None):
        """n_frames raw Bayer mosaics of width x height samples at d_src (bytes, or 16-bit words when params.bits > 8) demosaiced
        into the device frames at d_dst in format fmt (default: the input format): black level and white balance on each sample,
        bilinear interpolation at full depth with reflected borders, the reduction to 8 bits (params: bayer_params(...); None: RGGB,
        8 bits, black 0, gains 1).  A four-channel destination gets byte 3 = 255, 'gray' the library's grey of the demosaiced
        colour.  Sides are 2 .. 32767, odd ones included, and are not bound by the detector's.  A source rectangle is d_src moved
        to its first sample with the full frame's strides and the pattern bayer_pattern_at(pattern, x0, y0).  The two sides must
        not overlap.  Needs no batch, allocates nothing, does not wait (stream None: the detector's own stream)."""
        sb = 2 if params is not None and params.bits > 8 else 1
        _, src_row_stride, src_frame_stride = self._strides(fmt, width, height, src_row_stride, src_frame_stride, bpp=sb)
        code, dst_row_stride, dst_frame_stride = self._strides(fmt, width, height, dst_row_stride, dst_frame_stride)
        self._check(self._lib.ocvar_hip_bayer_to_frames(self._ctx, d_src, src_row_stride, src_frame_stride, d_dst, dst_row_stride,
                                                        dst_frame_stride, width, height, n_frames, code,
                                                        None if params is None else C.byref(params), stream), "bayer_to_frames")

    def warp(self, d_src, src_width, src_height, d_dst, dst_width, dst_height, n_frames, d_maps, interp="linear", border="constant", fill=None,
             inverse_map=False, one_map=False, fmt=None, src_row_stride=None, src_frame_stride=None, dst_row_stride=None,
             dst_frame_stride=None, d_status_ptr=None, stream=None):
        """n_frames device frames of src_width x src_height pixels at d_src in format fmt (default: the input format) warped into the
        device frames of dst_width x dst_height at d_dst by the projective maps at d_maps: float64 [n_frames, 9] in device memory
        ([9] with one_map), the forward maps from source to destination pixels as OpenCV's warpPerspective takes them (perspective_map
        makes one), or with inverse_map the maps from destination to source pixels (board_plane_maps writes those).  interp 'linear'
        or 'nearest'; border 'constant' (taps outside the source read fill, up to four bytes in the format's memory order, default
        zeros) or 'replicate'.  d_status_ptr: device ints [n_frames], 1 where the frame was warped, 0 where its map is not finite or
        singular -- such a frame's destination bytes are not touched.  The sizes are not bound by the detector's.  Source and
        destination must not overlap.  Needs no batch, does not wait (stream None: the detector's own stream)."""
        if not (isinstance(interp, str) and interp.lower() in WARP_INTERPS):
            raise ValueError(f"unknown interpolation {interp!r}: one of {sorted(WARP_INTERPS)}")
        if not (isinstance(border, str) and border.lower() in WARP_BORDERS):
            raise ValueError(f"unknown border {border!r}: one of {sorted(WARP_BORDERS)}")
        code, src_row_stride, src_frame_stride = self._strides(fmt, src_width, src_height, src_row_stride, src_frame_stride)
        code, dst_row_stride, dst_frame_stride = self._strides(fmt, dst_width, dst_height, dst_row_stride, dst_frame_stride)
        fill4 = None
        if fill is not None:
            f = [int(v) for v in np.atleast_1d(fill)]
            if len(f) > 4 or any(v < 0 or v > 255 for v in f):
                raise ValueError("fill: up to four bytes")
            fill4 = (C.c_uint8 * 4)(*(f + [0] * (4 - len(f))))
        flags = (WARP_INVERSE_MAP if inverse_map else 0) | (WARP_ONE_MAP if one_map else 0)
        self._check(self._lib.ocvar_hip_warp(self._ctx, d_src, src_width, src_height, src_row_stride, src_frame_stride, d_dst, dst_width,
                                             dst_height, dst_row_stride, dst_frame_stride, n_frames, code, d_maps, WARP_INTERPS[interp.lower()],
                                             WARP_BORDERS[border.lower()], fill4, flags, d_status_ptr, stream), "warp")

    def warp_records(self, d_markers, d_counts, n_frames, d_out, d_maps, per_frame=None, one_map=False, pose=False, stream=None):
        """the squares of the device records [n_frames, per_frame] (default per_frame: max_markers) under counts [n_frames] carried
        through the forward maps at d_maps (float64 [n_frames, 9] in device memory, [9] with one_map) to where warp(...) puts those
        frames' pixels, every other field copied, into the device records at d_out (which may be d_markers); slots at or beyond a
        frame's count are not written; a corner the map sends to infinity becomes NaN.  pose: glMatrix is solved again from the new
        square with the camera set at the call, which must be that of the warped frames.  Needs no batch, does not wait (stream None:
        the detector's own stream)."""
        per_frame = self.max_markers if per_frame is None else per_frame
        flags = (WARP_ONE_MAP if one_map else 0) | (WARP_POSE if pose else 0)
        self._check(self._lib.ocvar_hip_warp_records(self._ctx, d_markers, d_counts, n_frames, per_frame, d_maps, flags, d_out, stream),
                    "warp_records")

    def board_plane_maps(self, d_poses_ptr, n_frames, rect, dst_width, dst_height, d_maps, stream=None):
        """for the n_frames board poses in device memory at d_poses_ptr (board_poses_to_device) the maps, float64 [n_frames, 9] into
        the device memory at d_maps, that show the rectangle rect = (x0, y0, x1, y1) of the board's plane (board units) from straight
        above in frames of dst_width x dst_height pixels: pixel (0, 0) is board point (x0, y0), pixel (dst_width - 1, dst_height - 1)
        is (x1, y1) -- flip the picture by choosing y0 > y1.  They map destination to source pixels: warp(..., inverse_map=True).  The
        camera matrix is the one set at the call; the lens is ignored, so undistort the frames first.  A frame without a solved pose
        gets nine NaNs and warp skips it (status 0).  Needs no batch, does not wait (stream None: the detector's own stream)."""
        r = (C.c_double * 4)(*[float(v) for v in rect])
        self._check(self._lib.ocvar_hip_board_plane_maps(self._ctx, d_poses_ptr, n_frames, r, dst_width, dst_height, d_maps, stream),
                    "board_plane_maps")

    def flow_records(self, d_prev, d_next, width, height, n_frames, d_markers, d_counts, d_out, per_frame=None, fmt=None,
                     prev_row_stride=None, prev_frame_stride=None, next_row_stride=None, next_frame_stride=None, params=None, pose=False,
                     d_status_ptr=None, d_err_ptr=None, stream=None):
        """the device records [n_frames, per_frame] (default per_frame: max_markers) under counts [n_frames], found on the n_frames
        device frames at d_prev, carried to the frames at d_next in format fmt (default: the input format) by pyramidal Lucas-Kanade
        on their corners, into the device records at d_out (which may be d_markers): a tracked record (status 1) has its square
        replaced -- and with pose (or params made with pose=True) its glMatrix solved from it with the camera set at the call --,
        a failed one (status -1 .. -6: include/ocvar_hip.h) is copied unchanged; slots at or beyond a frame's count get status 0 and
        are not written.  params: flow_params(...), default the library's.  d_status_ptr: device ints [n_frames, per_frame];
        d_err_ptr: device floats [n_frames, per_frame, 4], the corners' mean absolute differences.  Needs no batch, does not wait
        (stream None: the detector's own stream); the frames are only read."""
        per_frame = self.max_markers if per_frame is None else per_frame
        code, prev_row_stride, prev_frame_stride = self._strides(fmt, width, height, prev_row_stride, prev_frame_stride)
        code, next_row_stride, next_frame_stride = self._strides(fmt, width, height, next_row_stride, next_frame_stride)
        p = flow_params() if params is None else FlowParams.from_buffer_copy(bytes(params))
        if pose:
            p.flags |= FLOW_POSE
        self._check(self._lib.ocvar_hip_flow_records(self._ctx, d_prev, prev_row_stride, prev_frame_stride, d_next, next_row_stride,
                                                     next_frame_stride, width, height, n_frames, code, d_markers, d_counts, per_frame,
                                                     C.byref(p), d_out, d_status_ptr, d_err_ptr, stream), "flow_records")

    TUNE = {"crop_phases": 1, "mid_steps": 2, "mid_blocks": 3, "long_blocks": 4, "short_blocks": 5, "min_units": 6, "hp_mask": 7, "gate_mode": 8,
            "warp_direct": 9, "bayer_pairs": 10}

    def set_tuning(self, **kw):
        """result-invariant launch parameters (include/ocvar_hip.h: OCVAR_TUNE_*); 0 restores a default"""
        for k, v in kw.items():
            self._check(self._lib.ocvar_hip_set_tuning(self._ctx, self.TUNE[k], int(v)), f"set_tuning({k})")

    def set_gate(self, gate):
        """share a Gate with other detectors on the same GPU (None removes it); the detector keeps the gate alive"""
        self._check(self._lib.ocvar_hip_set_gate(self._ctx, gate._g if gate is not None else None), "set_gate")
        self._gate = gate

    def results_to_device(self, d_markers_ptr, d_counts_ptr, stream=None, per_frame=None):
        """Copies the enqueued batch's [n][per_frame] marker records (the first per_frame of every frame) and [n] full counts
        into caller-owned device buffers (stream-ordered), e.g. torch tensors handed to an RCCL gather (default per_frame:
        max_markers)."""
        per_frame = self.max_markers if per_frame is None else per_frame
        self._check(self._lib.ocvar_hip_results_to_device_ex(self._ctx, d_markers_ptr, d_counts_ptr, per_frame, stream), "results_to_device")

    def detect_device(self, d_ptr, width, height, n_frames, **kw):
        max_per_frame = kw.pop("max_per_frame", None)
        self.enqueue_device(d_ptr, width, height, n_frames, **kw)
        return self.collect(max_per_frame)

    def detect_host(self, frames, grey_in_place=False, prev=None, max_per_frame=None):
        """frames: uint8 array (C-contiguous) [n, H, W, 3] (bgr, rgb), [n, H, W, 4] (bgra, rgba) or [n, H, W] (gray), as the
        input format says.  Greyed in place when asked (reference side effect; a gray frame is left as it is)."""
        assert frames.dtype == np.uint8 and frames.flags.c_contiguous
        max_per_frame = self.max_markers if max_per_frame is None else max_per_frame
        n, h, w = frame_shape_bpp(frames.shape, self.input_format)
        bpp = FORMAT_BPP[self.input_format]
        markers = np.zeros((n, max_per_frame), MARKER_DTYPE)
        counts = np.zeros(n, np.int32)
        pm, pc = self._prev_arrays(prev, n)
        self._check(self._lib.ocvar_hip_detect_host(self._ctx, _ptr(frames), w, h, bpp * w, bpp * w * h, n, int(grey_in_place),
                                                    _ptr(pm), _ptr(pc), _ptr(markers), _ptr(counts), max_per_frame),
                    "detect_host")
        self._n = n
        return markers, counts

    def find_squares(self, gray):
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        h, w = g.shape
        mq = self.max_quads
        quads = np.zeros((mq, 4, 2), np.int32)
        n = C.c_int(0)
        self._check(self._lib.ocvar_hip_find_squares(self._ctx, _ptr(g), w, h, w, _ptr(quads), mq, C.byref(n)),
                    "find_squares")
        return quads[:min(n.value, mq)].copy(), n.value

    # parity hooks
    def debug_gray(self, frame, width, height):
        out = np.zeros((height, width), np.uint8)
        self._check(self._lib.ocvar_hip_debug_gray(self._ctx, frame, _ptr(out)), "debug_gray")
        return out

    def debug_binary(self, frame, width, height):
        out = np.zeros((height & -2, width & -2), np.uint8)
        self._check(self._lib.ocvar_hip_debug_binary(self._ctx, frame, _ptr(out)), "debug_binary")
        return out

    def debug_masks(self, frame, width, height):
        """8-neighbour masks of the frame pass (bit s: the neighbour in direction s = E,NE,N,NW,W,SW,S,SE is set), untiled."""
        out = np.zeros((height & -2, width & -2), np.uint8)
        self._check(self._lib.ocvar_hip_debug_masks(self._ctx, frame, _ptr(out)), "debug_masks")
        return out

    def debug_frame_quads(self, frame):
        quads = np.zeros((MAX_QUADS, 4, 2), np.int32)
        n = C.c_int(0)
        self._check(self._lib.ocvar_hip_debug_frame_quads(self._ctx, frame, _ptr(quads), C.byref(n)), "debug_frame_quads")
        return quads[:min(n.value, MAX_QUADS)].copy()

    def debug_candidates(self, frame, max_cands=None):
        """the pre-dedupe candidates of batch position `frame` (all of them by default: the frame's squares x n_templates at most)"""
        n = C.c_int(0)
        if max_cands is None:
            one = (Candidate * 1)()
            self._check(self._lib.ocvar_hip_debug_candidates(self._ctx, frame, one, 1, C.byref(n)), "debug_candidates")
            max_cands = max(n.value, 1)
        arr = (Candidate * max_cands)()
        self._check(self._lib.ocvar_hip_debug_candidates(self._ctx, frame, arr, max_cands, C.byref(n)), "debug_candidates")
        return [arr[i] for i in range(min(n.value, max_cands))]

    def debug_crops(self):
        """the crop ROIs of the last collected batch, [n] CROP_ROI_DTYPE (index, frame, owner = index of the frame-pass square,
        x0, y0, w, h), in the batch's own order; valid until the next enqueue"""
        n = C.c_int(0)
        self._check(self._lib.ocvar_hip_debug_crop_rois(self._ctx, None, 0, C.byref(n)), "debug_crop_rois")
        out = np.zeros(max(n.value, 1), CROP_ROI_DTYPE)
        self._check(self._lib.ocvar_hip_debug_crop_rois(self._ctx, _ptr(out), n.value, C.byref(n)), "debug_crop_rois")
        return out[:n.value]

    def _debug_crop_plane(self, roi, masks):
        # the buffer is sized by the ROI as the context holds it now: a record kept from an earlier batch is refused
        rois = self.debug_crops()
        r = rois[int(roi["index"]) if isinstance(roi, np.void) else int(roi)]   # (IndexError for an index past the list)
        if isinstance(roi, np.void) and roi != r:
            raise ValueError("debug_crop_plane: the record is not of the last collected batch")
        out = np.zeros((int(r["h"]) & -2, int(r["w"]) & -2), np.uint8)
        self._check(self._lib.ocvar_hip_debug_crop_plane(self._ctx, int(r["index"]), int(masks), _ptr(out)), "debug_crop_plane")
        return out

    def debug_crop_binary(self, roi):
        """the binary image (0 / 255, the 1-px frame zero) of crop `roi` -- an index into debug_crops() or one of its records --
        of the last collected batch, (h & ~1) x (w & ~1)"""
        return self._debug_crop_plane(roi, False)

    def debug_crop_masks(self, roi):
        """the 8-neighbour masks of crop `roi`, as debug_masks gives a frame's"""
        return self._debug_crop_plane(roi, True)

    def debug_starts(self, crop_pass=False):
        """the border starts the binarise kernel of the last collected batch's frame pass (or crop pass) handed to the followers,
        [n] START_DTYPE (roi = frame of the batch or index into debug_crops(), x, y, is_hole); the order differs from run to run"""
        n = C.c_int(0)
        self._check(self._lib.ocvar_hip_debug_starts(self._ctx, int(bool(crop_pass)), None, 0, C.byref(n)), "debug_starts")
        out = np.zeros(max(n.value, 1), START_DTYPE)
        self._check(self._lib.ocvar_hip_debug_starts(self._ctx, int(bool(crop_pass)), _ptr(out), n.value, C.byref(n)), "debug_starts")
        return out[:n.value]

    def debug_rings(self, crop_pass=False):
        """the ring verdicts of the last collected batch, int32 [frames of the batch], or [len(debug_crops())] indexed like its
        `index`: 1 where ring_quads_kernel found the ring next to the ROI's zeroed frame all set (tier 1 then drops the border that
        begins at (1, 1)); all zeros after a batch of at most 8 frames"""
        n = C.c_int(0)
        self._check(self._lib.ocvar_hip_debug_rings(self._ctx, int(bool(crop_pass)), None, 0, C.byref(n)), "debug_rings")
        out = np.zeros(max(n.value, 1), np.int32)
        self._check(self._lib.ocvar_hip_debug_rings(self._ctx, int(bool(crop_pass)), _ptr(out), n.value, C.byref(n)), "debug_rings")
        return out[:n.value]

    def stage_ms(self):
        ms = np.zeros(12, np.float32)
        k = self._lib.ocvar_hip_stage_ms(self._ctx, _ptr(ms), 12)
        return ms[:max(k, 0)]

    def stream_ptr(self):
        """the context's own hipStream_t as an integer (torch.cuda.ExternalStream(ptr) wraps it)"""
        return self._lib.ocvar_hip_stream(self._ctx)

    def stage_stamps(self, ref_event):
        """the 13 stage boundaries of the last batch in ms after ref_event (a raw hipEvent_t, e.g. torch.cuda.Event(enable_timing=True).cuda_event)"""
        ms = np.zeros(13, np.float32)
        k = self._lib.ocvar_hip_stage_stamps(self._ctx, ref_event, _ptr(ms), 13)
        return ms[:max(k, 0)]

    def counters(self, n=10):
        """work counters of the last batch (n = 42 adds the profiling slots of a -DOCVAR_PROF build)"""
        out = np.zeros(n, np.int64)
        k = self._lib.ocvar_hip_counters(self._ctx, _ptr(out), n)
        return out[:max(k, 0)]
