"""The warp core (opencv-ar_amd/csrc/warp_core.h) in its host build (tests/emul/warp_emul.cpp), without a GPU: the sampler against a
numpy restatement byte for byte, the identity and a translation, equivalence with the patch extraction's pinned definition, skipped
frames, the record map, the board's plane map, the tile plan, the bird's-eye chain through the oracle, the stand-alone program under
the sanitizers, and the ABI.  tests/test_gpu_warp.py holds the kernels to this build byte for byte."""
import os
import re

import numpy as np
import pytest

import board_chain as BC
import frame_kit as FK
import helpers as H
import persp_synth as PS
import warp_chain as WC
from hostbuild import run_sanitized

CHAIN_MEASURED_PX, CHAIN_BAR_PX, CHAIN_SCENES = WC.CHAIN_MEASURED_PX, WC.CHAIN_BAR_PX, WC.CHAIN_SCENES


@pytest.fixture(scope="module")
def L():
    return WC.build_emul()


def image(rng, w, h, ch):
    return rng.integers(0, 256, (h, w, ch), dtype=np.uint8)


def test_constants_agree_with_the_core(L):
    assert (L.warp_tile_w_emul(), L.warp_lds_dwords_emul()) == (WC.TILE_W, WC.LDS_DWORDS)
    assert {bpp: L.warp_tile_h_emul(bpp) for bpp in (1, 3, 4)} == WC.TILE_HS


# ---- the sampler against numpy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
def test_frames_against_numpy(L, fmt):
    """guarded frames with padded rows, aligned and odd layouts, every shared map, both interpolations, both borders, a fill that is
    not zero: numpy's pixels and status, every guard byte kept, the source untouched"""
    src_size, dst_size = (37, 23), (45, 29)
    maps = WC.shared_maps(src_size, dst_size)
    names = list(maps)
    fill = [7, 130, 255, 66]
    for k, (interp, border) in enumerate([(i, b) for i in (WC.LINEAR, WC.NEAREST) for b in (WC.CONSTANT, WC.REPLICATE)]):
        aligned = k % 2 == 0
        for inverse in (0, WC.INVERSE_MAP):
            use = [n for n in names if maps[n][1] == inverse]
            src = FK.pix_layout(len(use), *src_size, fmt, aligned, seed=k + 1)
            dst = WC.dst_layout(src, dst_size, aligned)
            rc, got, status = WC.host_warp(L, src, dst, [maps[n][0] for n in use], interp, border, fill, inverse)
            assert rc == len(use) and status.tolist() == [1] * len(use)
            assert (got[~dst.pixel_mask()] == FK.GUARD).all()
            for f, n in enumerate(use):
                want, st = WC.np_warp(src.view(f), maps[n][0], dst_size, interp, border, fill, inverse)
                assert st == 1
                bad = np.argwhere(dst.view(f, got) != want)
                assert bad.size == 0, (fmt, n, interp, border, bad[:4].tolist())


def test_tiny_frames_against_numpy(L):
    """sources and destinations of 1 x 1 and 2 x 1 pixels, and a source narrower than a dword"""
    rng = np.random.default_rng(5)
    for (sw, sh), (dw, dh) in [((1, 1), (1, 1)), ((2, 1), (1, 1)), ((1, 1), (2, 1)), ((2, 1), (2, 1)), ((3, 1), (5, 2)), ((1, 3), (2, 5))]:
        for ch in (1, 3, 4):
            img = image(rng, sw, sh, ch)
            for m, flags in [(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0]), 0), (np.array([0.5, 0, 0.25, 0, 0.5, 0.125, 0, 0, 1.0]), WC.INVERSE_MAP),
                             (np.array([1, 0, -0.5, 0, 1, 0, 0.25, 0, 1.0]), WC.INVERSE_MAP)]:
                for interp in (WC.LINEAR, WC.NEAREST):
                    for border in (WC.CONSTANT, WC.REPLICATE):
                        got, st = WC.host_warp_image(L, img, m, (dw, dh), interp, border, [1, 2, 3, 4], flags)
                        want, st2 = WC.np_warp(img, m, (dw, dh), interp, border, [1, 2, 3, 4], flags)
                        assert st == st2 == 1 and (got == want).all(), ((sw, sh), (dw, dh), ch, m.tolist(), interp, border)


@pytest.mark.parametrize("interp", [WC.LINEAR, WC.NEAREST])
def test_identity_copies_the_frame(L, interp):
    rng = np.random.default_rng(1)
    for ch in (1, 3, 4):
        img = image(rng, 70, 19, ch)
        for flags in (0, WC.INVERSE_MAP):
            for border in (WC.CONSTANT, WC.REPLICATE):
                got, st = WC.host_warp_image(L, img, [1, 0, 0, 0, 1, 0, 0, 0, 1], (70, 19), interp, border, [200, 100, 50, 25], flags)
                assert st == 1 and (got == img).all()


@pytest.mark.parametrize("interp", [WC.LINEAR, WC.NEAREST])
def test_integer_translation_shifts_and_fills(L, interp):
    """the forward map x' = x + 3, y' = y - 2: pixels move by (3, -2), the rest is the fill, or the nearest edge pixel"""
    rng = np.random.default_rng(2)
    img = image(rng, 40, 21, 3)
    m = [1, 0, 3, 0, 1, -2, 0, 0, 1]
    fill = [11, 22, 33]
    got, _ = WC.host_warp_image(L, img, m, (40, 21), interp, WC.CONSTANT, fill)
    want = np.empty_like(img)
    want[...] = np.array(fill, np.uint8)
    want[:19, 3:] = img[2:, :37]
    assert (got == want).all()
    got, _ = WC.host_warp_image(L, img, m, (40, 21), interp, WC.REPLICATE)
    ys, xs = np.clip(np.arange(21) + 2, 0, 20), np.clip(np.arange(40) - 3, 0, 39)
    assert (got == img[ys][:, xs]).all()


# ---- the pinned definition --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bgr", "rgba", "gray"])
def test_a_warp_is_the_patch_of_the_same_quad(L, fmt):
    """forward map perspective_from_quad(square, pw, ph) widened to double, destination pw x ph, CONSTANT border with fill 0: the bytes
    of patch_extract_frame, for quads inside, across and outside the frame"""
    rng = np.random.default_rng(3)
    W, Hh = 160, 120
    code, ch = FK.FORMATS[fmt], FK.BPP[FK.FORMATS[fmt]]
    img = np.ascontiguousarray(image(rng, W, Hh, ch))
    quads = [[20, 15, 90, 25, 100, 95, 12, 80], [-30, -20, 60, 10, 70, 70, -10, 90], [100, 60, 200, 50, 210, 160, 90, 150],
             [40.5, 30.25, 44.75, 31, 45, 36.5, 39, 35], [300, 300, 400, 300, 400, 400, 300, 400]]
    sizes = [(64, 64), (33, 17), (2, 2), (65, 129), (256, 3)]
    for q, (pw, ph) in zip(quads, sizes):
        rec = FK.records([q])
        patch = np.full((ph, pw, ch), 0x5A, np.uint8)
        m = np.zeros(9)
        st = L.warp_patch_reference_emul(img.ctypes.data, W, Hh, W * ch, code, rec.ctypes.data, pw, ph, patch.ctypes.data, m.ctypes.data)
        assert st == 1 and m[8] == 1.0
        got, wst = WC.host_warp_image(L, img, m, (pw, ph), WC.LINEAR, WC.CONSTANT, None, 0, background=0x5A)
        assert wst == 1 and (got == patch).all(), (q, pw, ph, np.argwhere(got != patch)[:4].tolist())
    assert (patch == 0).all()     # (the last quad lies outside the frame)


# ---- skipped frames -----------------------------------------------------------------------------------------------------------------------

def test_skipped_frames_keep_their_bytes(L):
    """maps that are not finite or singular among good ones: status 0 and every byte of those frames untouched, the others warped"""
    names = list(WC.SKIPPED_MAPS)
    good = WC.about_centre((20, 12), (24, 10), 1.2, 8.0)
    maps = [good] + [WC.SKIPPED_MAPS[n] for n in names] + [good]
    for flags in (0, WC.INVERSE_MAP):
        src = FK.pix_layout(len(maps), 20, 12, "bgr", False, seed=9)
        dst = WC.dst_layout(src, (24, 10), False)
        rc, got, status = WC.host_warp(L, src, dst, maps, WC.LINEAR, WC.CONSTANT, [1, 2, 3], flags)
        skipped = [0] + [0 if (flags == 0 or not np.isfinite(WC.SKIPPED_MAPS[n]).all()) else 1 for n in names] + [0]
        skipped[0] = skipped[-1] = 1
        assert status.tolist() == skipped and rc == sum(skipped)
        assert (got[~dst.pixel_mask()] == FK.GUARD).all()
        for f in range(len(maps)):
            if status[f] == 0:
                assert (dst.view(f, got) == FK.GUARD).all()
            else:
                want, st = WC.np_warp(src.view(f), maps[f], (24, 10), WC.LINEAR, WC.CONSTANT, [1, 2, 3], flags)
                assert st == 1 and (dst.view(f, got) == want).all()
        for n in names:
            ok, _ = WC.host_map(L, WC.SKIPPED_MAPS[n], 0)
            assert not ok and WC.np_invert(WC.SKIPPED_MAPS[n]) is None, n
    assert L.warp_emul(None, 4, 4, 12, 48, None, 4, 4, 12, 48, 1, 0, None, 2, 0, None, 0, None) == FK.E_ARG
    assert L.warp_emul(None, 4, 4, 12, 48, None, 4, 4, 12, 48, 1, 0, None, 1, 2, None, 0, None) == FK.E_ARG
    assert L.warp_emul(None, 4, 4, 12, 48, None, 4, 4, 12, 48, 1, 0, None, 1, 0, None, 4, None) == FK.E_ARG
    assert L.warp_emul(None, 4, 4, 12, 48, None, 4, 32768, 12, 48, 1, 0, None, 1, 0, None, 0, None) == FK.E_ARG
    assert L.warp_emul(None, 4, 4, 12, 48, None, 4, 4, 12, 48, 1, 5, None, 1, 0, None, 0, None) == FK.E_ARG


# ---- records --------------------------------------------------------------------------------------------------------------------------

def test_record_map_against_numpy(L):
    """random, huge, infinite and NaN coordinates and corners on the horizon through known homographies: the float64 numpy map's
    bits, NaN in the one bit pattern, w = 0 giving NaN; every other field and every slot at or beyond the count untouched; into the
    block itself and into another one"""
    rng = np.random.default_rng(4)
    n, slots = 3, 6
    maps = np.stack([WC.about_centre((640, 480), (800, 600), 1.3, 20.0, 1e-4, -2e-4), np.array([2, 0, 1, 0, 2, 3, 1, 0, -0.25]),
                     np.array([1, 2, 3, 2, 4, 6, 0, 0, 1.0])])
    recs = np.zeros((n, slots), FK.MARKER_DTYPE)
    recs["square"] = rng.uniform(-50, 700, (n, slots, 8)).astype(np.float32)
    recs["glMatrix"] = rng.normal(size=(n, slots, 16))
    recs["templateId"] = rng.integers(0, 9, (n, slots))
    recs["score"] = rng.integers(0, 2, (n, slots))
    recs["aspectRatio"] = rng.uniform(0.5, 2, (n, slots))
    recs["square"][0, 0, :4] = [np.nan, 1, np.inf, -np.inf]
    recs["square"][0, 1, :2] = [1e30, -1e30]
    recs["square"][1, 0, :2] = [0.25, 9]            # w = x - 0.25 = 0
    recs["square"][1, 1, :2] = [0.25, -1e9]
    counts = np.array([slots, 2, slots + 3], np.int32)
    live = np.arange(slots)[None, :] < np.minimum(counts, slots)[:, None]
    want_sq = np.stack([WC.np_warp_squares(recs["square"][f], maps[f]) for f in range(n)])
    assert want_sq.view(np.uint32)[1, 0, 0] == WC.NAN_BITS and want_sq.view(np.uint32)[1, 1, 1] == WC.NAN_BITS and want_sq.view(np.uint32)[0, 0, 0] == WC.NAN_BITS
    for out in (None, np.frombuffer(np.full(recs.nbytes, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(n, slots)):
        rc, got = WC.host_warp_records(L, recs, counts, maps, 0, out=out)
        assert rc == 0
        want = (recs if out is None else out).copy()
        want[live] = recs[live]
        want["square"][live] = want_sq[live]
        assert got.tobytes() == want.tobytes()
    rc, one = WC.host_warp_records(L, recs, counts, maps[:1], WC.ONE_MAP)
    assert rc == 0 and one["square"][live].view(np.uint32).tolist() == np.stack([WC.np_warp_squares(recs["square"][f], maps[0]) for f in range(n)])[live].view(np.uint32).tolist()
    for flags in (WC.INVERSE_MAP, WC.POSE, 8, -1):     # (POSE: no camera given)
        before = recs.copy()
        rc, got = WC.host_warp_records(L, recs, counts, maps, flags)
        assert rc == FK.E_ARG and got.tobytes() == before.tobytes()


def test_records_follow_the_pixels_and_the_pose_flag(L):
    """a record's corners land where the warp puts those pixels (the forward map of the frame call), and with OCVAR_WARP_POSE the new
    glMatrix reprojects the model corners onto the new square under the camera"""
    import orient_chain as OR
    size = (640, 480)
    cam = PS.camera(*size)
    # a square seen by the camera, and the homography K Rc K^-1 a turn Rc of the camera induces: the new view has a rigid pose
    K = np.array(list(cam.cameraMatrix)).reshape(3, 3)
    m = (K @ BC.rodrigues(np.array([0.05, -0.08, 0.2])) @ np.linalg.inv(K)).reshape(9)
    sq = PS.project(cam, *PS.pose(cam, 300, 250, 110, 25, 30, 40)).reshape(1, 8).astype(np.float32)
    recs = FK.records(sq).reshape(1, 1)
    recs["aspectRatio"] = 1.0
    rc, got = WC.host_warp_records(L, recs, [1], m, WC.POSE, cam=cam)
    assert rc == 0
    new = got["square"][0, 0].reshape(4, 2).astype(np.float64)
    assert np.abs(new - WC.apply_map(m, sq.reshape(4, 2))).max() <= 1e-4
    ok, M = WC.host_map(L, m)
    assert ok and np.abs(WC.apply_map(M, new) - sq.reshape(4, 2)).max() <= 1e-3     # the frame call reads those source pixels there
    assert np.abs(OR.gl_reprojection(got["glMatrix"][0, 0], cam, 1.0) - new).max() <= 0.05
    assert (got["glMatrix"][0, 0] != recs["glMatrix"][0, 0]).any()


# ---- the board's plane ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def board_scenes():
    cam = PS.camera(1920, 1080)
    names, board, sc = WC.chain_scenes(CHAIN_SCENES, cam)
    return dict(names=names, board=board, scenes=sc, cam=cam)


def test_the_cores_own_sine_and_cosine(L):
    """warp_sincos, which keeps the plane maps free of the math libraries' last bits: within 1 ulp of the library's values (which are
    within 1 ulp of the true ones) on 0 .. 2 pi and at the quarter turns, to 1e-12 up to a hundred turns"""
    import math
    out = np.zeros(2)
    rng = np.random.default_rng(7)
    worst = 0.0
    quarter = [k * math.pi / 2 for k in range(9)]
    for th in [0.0, 1e-300, 1e-9, math.pi / 4, 0.7853981633974484] + quarter + list(rng.uniform(0, 2 * math.pi, 4000)) + list(rng.uniform(0, 1e-3, 200)):
        L.warp_sincos_emul(th, out.ctypes.data)
        for got, want in ((out[0], math.sin(th)), (out[1], math.cos(th))):
            worst = max(worst, abs(got - want) / max(np.spacing(abs(want)), np.spacing(0.25)))
    assert worst <= 2.0, worst          # in units of the last place of the value, or of 0.25 for values below it
    for th in rng.uniform(0, 200 * math.pi, 500):
        L.warp_sincos_emul(th, out.ctypes.data)
        assert abs(out[0] - math.sin(th)) <= 1e-12 and abs(out[1] - math.cos(th)) <= 1e-12


def test_plane_map_lands_on_the_pinhole_projection(L, board_scenes):
    """poses of board_chain's scenes: the four corners of rect, as destination pixels through the map, land on the pinhole projection
    of the same board points to 1e-9 px; a flipped rectangle, a 1-pixel destination; status 0, NaN and a flat rectangle give NaNs"""
    b = board_scenes
    K = np.array(list(b["cam"].cameraMatrix)).reshape(3, 3)
    for _, _, R, t in b["scenes"]:
        pose = WC.board_pose(R, t)
        Rr = BC.rodrigues(np.array(pose.rvec))
        for rect, size in [((-0.5, -0.5, 6.0, 4.5), (521, 401)), ((0, 4, 5.5, 0), (300, 200)), ((1, 1, 2, 2), (1, 1)), ((1, 1, 1, 3), (1, 7))]:
            M = WC.host_plane_maps(L, [pose], K, rect, size)[0]
            assert np.isfinite(M).all()
            px = np.array([[0, 0], [size[0] - 1, 0], [size[0] - 1, size[1] - 1], [0, size[1] - 1]], np.float64)
            x0, y0, x1, y1 = rect
            pts = np.array([[x0, y0], [x1 if size[0] > 1 else x0, y0], [x1 if size[0] > 1 else x0, y1 if size[1] > 1 else y0], [x0, y1 if size[1] > 1 else y0]], np.float64)
            want = BC.project(K, np.zeros(5), Rr, np.array(pose.tvec), pts)
            assert np.abs(WC.apply_map(M, px) - want).max() <= 1e-9, (rect, size)
            scale = np.abs(M).max()
            assert np.abs(M - WC.np_plane_map(Rr, np.array(pose.tvec), K, rect, size)).max() <= 1e-12 * scale
    R, t = b["scenes"][0][2], b["scenes"][0][3]
    bad = [WC.board_pose(R, t, status=0), WC.board_pose(R, t, status=-1), WC.board_pose(R, [np.nan, 0, 5]), WC.board_pose(R, [0, np.inf, 5])]
    M = WC.host_plane_maps(L, bad + [WC.board_pose(R, t)], K, (0, 0, 5, 4), (64, 48))
    assert np.isnan(M[:4]).all() and np.isfinite(M[4]).all()
    for rect, size in [((1, 0, 1, 4), (64, 48)), ((0, 2, 5, 2), (64, 48)), ((0, 0, np.nan, 4), (64, 48)), ((0, 0, 5, np.inf), (64, 48))]:
        assert np.isnan(WC.host_plane_maps(L, [WC.board_pose(R, t)], K, rect, size)).all(), rect
    # and the warp skips such a frame
    ok, _ = WC.host_map(L, M[0], WC.INVERSE_MAP)
    assert not ok


# ---- the tile plan ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(WC.PLAN_CASES))
def test_tile_plan_windows_hold_every_tap(L, case):
    """for the maps of the GPU test: no tap of a pixel of a staged tile lies outside the tile's window, the image fits the LDS budget,
    and the case shows the classes it claims -- at least one tile of each where it claims both"""
    src_size, dst_size, name, classes = WC.PLAN_CASES[case]
    m, flags = WC.shared_maps(src_size, dst_size)[name]
    for bpp in (1, 3, 4):
        for interp in (WC.LINEAR, WC.NEAREST):
            for border in (WC.CONSTANT, WC.REPLICATE):
                c = WC.plan_counts(L, m, src_size, dst_size, bpp, interp, border, flags)
                tiles = -(-dst_size[0] // WC.TILE_W) * -(-dst_size[1] // WC.TILE_HS[bpp])
                assert c["ok"] == 1 and c["staged"] + c["direct"] == tiles
                assert c["missed"] == 0 and c["words"] <= WC.LDS_DWORDS, (case, bpp, c)
                if classes == "staged":
                    assert c["direct"] == 0 and c["staged"] >= 1, (case, bpp, c)
                elif classes == "direct":
                    assert c["staged"] == 0 and c["direct"] >= 1, (case, bpp, c)
                else:
                    assert c["staged"] >= 1 and c["direct"] >= 1, (case, bpp, c)
                if c["staged"]:
                    assert c["taps"] > 0 or name == "outside"


def test_tile_plan_rules(L):
    """one tile at a time: the window of the identity is the tile grown by the margin and clamped into the frame; w through 0 on a
    corner, a sign change, a NaN, a far corner and a window over the budget are direct; the budget is the only thing that depends on
    the pixel size"""
    out = np.zeros(8, np.int32)
    I = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0])

    def plan(M, tile, src, bpp=3, interp=WC.LINEAR, budget=WC.LDS_DWORDS):
        L.warp_tile_plan_emul(np.ascontiguousarray(M, np.float64).ctypes.data, *tile, *src, bpp, interp, budget, out.ctypes.data)
        return dict(zip(["staged", "x0", "y0", "w", "h", "b0", "row_dwords", "pitch"], out.tolist()))

    p = plan(I, (64, 16, 64, 16), (1000, 500))
    # columns 64 .. 127 and their right neighbours 128: floor + 1, + 1 for the far taps, +- 1 margin: 63 .. 130
    assert (p["staged"], p["x0"], p["y0"], p["w"], p["h"]) == (1, 63, 15, 68, 20)
    assert p["b0"] == (63 * 3) & ~3 and p["row_dwords"] == (131 * 3 + 3 - p["b0"]) // 4 and p["pitch"] % 2 == 1 and p["pitch"] > p["row_dwords"]
    p = plan(I, (64, 16, 64, 16), (1000, 500), interp=WC.NEAREST)
    assert (p["x0"], p["w"], p["h"]) == (63, 67, 19)
    p = plan(I, (0, 0, 64, 16), (10, 5))
    assert (p["staged"], p["x0"], p["y0"], p["w"], p["h"]) == (1, 0, 0, 10, 5)          # clamped into the frame
    p = plan(I, (640, 160, 64, 16), (10, 5))
    assert (p["staged"], p["x0"], p["y0"], p["w"], p["h"]) == (1, 9, 4, 1, 1)           # beyond the frame: where REPLICATE reads
    assert plan(I, (0, 0, 64, 16), (1000, 500), budget=0)["staged"] == 0
    assert plan(I, (0, 0, 64, 16), (1000, 500), bpp=4, budget=19 * 69 + 2)["staged"] == 1 and plan(I, (0, 0, 64, 16), (1000, 500), bpp=4, budget=19 * 69 + 1)["staged"] == 0
    for M in ([1, 0, 0, 0, 1, 0, 1, 0, -64.0], [1, 0, 0, 0, 1, 0, 1, 0, -80.0], [1, 0, 0, 0, 1, 0, 0, 0, np.nan], [1, 0, 1e7, 0, 1, 0, 0, 0, 1.0],
              [1, 0, 0, 0, 1, 0, 0, 0, 0.0]):
        assert plan(M, (64, 16, 64, 16), (1000, 500))["staged"] == 0, M
    assert plan([8, 0, 0, 0, 8, 0, 0, 0, 1.0], (0, 0, 64, 16), (1000, 500))["staged"] == 0        # 512 x 128 source pixels: over the budget
    assert plan([8, 0, 0, 0, 8, 0, 0, 0, 1.0], (0, 0, 64, 16), (1000, 500), bpp=1)["staged"] == 0


# ---- the chain, on the oracle only ------------------------------------------------------------------------------------------------------

def birds_eye(L, Lb, bgr, board, tpls, cam, rect, size, pose=None):
    """(the oracle's markers on the bird's-eye frame of one scene, the pose used): the host board core's pose from the oracle's
    records unless one is given, the plane map, the host warp"""
    if pose is None:
        _, _, pose, _, _ = BC.expected(None, Lb, bgr, board, tpls, cam)
        assert pose.status == 1 and pose.n_markers >= 6
    K = np.array(list(cam.cameraMatrix)).reshape(3, 3)
    M = WC.host_plane_maps(L, [pose], K, rect, size)[0]
    top, st = WC.host_warp_image(L, bgr, M, size, WC.LINEAR, WC.CONSTANT, [220, 220, 220], WC.INVERSE_MAP)
    assert st == 1
    found, _, _ = H.oracle_registration(top, tpls, PS.camera(*size))
    return found, pose


def test_the_birds_eye_chain_on_the_cpu(L, board_scenes):
    """a board (markers turned by 25 degrees in its plane) seen by a pinhole camera at tilts of 0 .. 50 degrees: the host board
    core's pose from the oracle's records, the plane map of the board's rectangle, the host warp to a bird's-eye frame -- on which the
    oracle's registration finds every marker of the board with the right template, its corners within CHAIN_BAR_PX of where the board
    layout and the rectangle put them.  Measured: 1.07 px at most (0.49 .. 1.07 per scene; 0.49 .. 0.62 with the true pose)."""
    b = board_scenes
    Lb = BC.build_emul()
    tpls = H.oracle_templates(b["names"])
    rect, size = WC.chain_rect(b["board"])
    worst = 0.0
    for i, (bgr, truth, R, t) in enumerate(b["scenes"]):
        found, _ = birds_eye(L, Lb, bgr, b["board"], tpls, b["cam"], rect, size)
        errs = WC.corner_errors(found, b["board"], rect, size)
        assert sorted(errs) == [tid for tid, _ in b["board"]], (i, sorted(errs))
        print("scene %d: %d markers, largest corner error %.3f px" % (i, len(errs), max(errs.values())))
        worst = max(worst, max(errs.values()))
        assert max(errs.values()) <= CHAIN_BAR_PX, (i, errs)
    print("bird's-eye chain: largest corner error %.3f px over %d scenes (bar %.2f)" % (worst, len(b["scenes"]), CHAIN_BAR_PX))
    assert worst <= CHAIN_MEASURED_PX       # the figure DESIGN.md states is what this chain gives


def test_axis_aligned_markers_in_the_birds_eye_frame(L):
    """board_chain's own board, whose markers stand axis-aligned in every bird's-eye frame: every marker is found with the right
    template.  On an axis-aligned square with straight edges the oracle's polygon approximation itself puts the corners (2, 1) px
    along the contour, sqrt(5) = 2.24 px off, under the TRUE pose -- an ideal rectification; that is the detector's own error on such
    frames and is held here as the finding it is.  The chain's bar on this board is therefore the ideal
    rectification's error plus one resampling's worth: under the solved pose no corner lies further off than that.  Measured:
    2.236 px with the solved pose and with the true pose, in both scenes."""
    cam = PS.camera(1920, 1080)
    names, board, sc = BC.scenes(2, cam=cam)
    Lb = BC.build_emul()
    tpls = H.oracle_templates(names)
    rect, size = WC.chain_rect(board)
    for i, (bgr, truth, R, t) in enumerate(sc):
        found, pose = birds_eye(L, Lb, bgr, board, tpls, cam, rect, size)
        ideal, _ = birds_eye(L, Lb, bgr, board, tpls, cam, rect, size, pose=WC.board_pose(R, t))
        errs, ideal_errs = WC.corner_errors(found, board, rect, size), WC.corner_errors(ideal, board, rect, size)
        assert sorted(errs) == sorted(ideal_errs) == [tid for tid, _ in board], (i, sorted(errs))
        print("scene %d: largest corner error %.3f px, with the true pose %.3f px" % (i, max(errs.values()), max(ideal_errs.values())))
        assert max(ideal_errs.values()) <= 5 ** 0.5 + 1e-9, (i, ideal_errs)         # the finding: the detector's pinwheel, no more
        assert max(errs.values()) <= max(ideal_errs.values()) + 1.0, (i, errs, ideal_errs)


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers():
    """tests/emul/warp_emul.cpp with its own main, built with -fsanitize=address,undefined and run as a program: sides 1 .. 32767,
    every pixel size, interpolation and border, maps that magnify, shrink, cross the horizon and miss the source, on heap blocks of
    exactly the bytes a call may touch"""
    run_sanitized("warp_emul", "WARP_EMUL_MAIN", ", 0 bad", timeout=600)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------

def test_abi_and_python_names():
    """the three entry points are declared in the header and exported by the library; the module's names agree with the header;
    perspective_map sends its four points where it says"""
    import __graft_entry__ as g
    g.build()
    import opencv_ar_amd as oa
    header = open(os.path.join(H.ROOT, "include", "ocvar_hip.h")).read()
    lib = oa.hip_lib()
    for name in ("ocvar_hip_warp", "ocvar_hip_warp_records", "ocvar_hip_board_plane_maps"):
        assert re.search(r"\bint %s\(" % name, header) and name in oa.HIP_SYMBOLS and hasattr(lib, name), name
    for name, value in [("NEAREST", 0), ("LINEAR", 1), ("BORDER_CONSTANT", 0), ("BORDER_REPLICATE", 1), ("INVERSE_MAP", 1), ("ONE_MAP", 2), ("POSE", 4)]:
        assert re.search(r"OCVAR_WARP_%s = %d\b" % (name, value), header), name
    assert oa.WARP_INTERPS == WC.INTERPS and oa.WARP_BORDERS == WC.BORDERS
    assert (oa.WARP_INVERSE_MAP, oa.WARP_ONE_MAP, oa.WARP_POSE) == (WC.INVERSE_MAP, WC.ONE_MAP, WC.POSE)
    assert re.search(r"OCVAR_TUNE_WARP_DIRECT = 9\b", header) and oa.Detector.TUNE["warp_direct"] == 9
    for n in ("warp", "warp_records", "board_plane_maps"):
        assert hasattr(oa.Detector, n)
    rng = np.random.default_rng(6)
    for _ in range(20):
        s = np.array([[0, 0], [100, 0], [100, 80], [0, 80]], np.float64) + rng.uniform(-20, 20, (4, 2))
        d = np.array([[10, 5], [300, 20], [280, 200], [-5, 190]], np.float64) + rng.uniform(-20, 20, (4, 2))
        m = oa.perspective_map(s, d)
        assert m.dtype == np.float64 and m.shape == (9,) and m[8] == 1.0
        assert np.abs(WC.apply_map(m, s) - d).max() <= 1e-8
    with pytest.raises(ValueError):
        oa.perspective_map([[0, 0], [1, 1], [2, 2], [0, 1]], [[0, 0], [1, 0], [1, 1], [0, 1]])
    with pytest.raises(ValueError):
        oa.perspective_map([[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 0], [1, 1], [0, 1]])
