"""Templates with width != height (tests/nonsquare_scenes.py) on the CPU: the host builds of the device's decode and pose cores
(tests/emul) against the oracle on every candidate and record of the 36 frames, under the planted library A and under the
extreme shapes of library B, and cvarLoadTemplateTag on non-square template files.

Poses are compared where the reference itself defines them (nonsquare_scenes.pose_is_defined); the tests print what they
measure (pytest -s)."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import nonsquare_scenes as NS
from helpers import P

HOST_RTOL = 1e-6   # host core against the oracle (the bar of tests/test_perspective_cpu.py)


@pytest.mark.parametrize("family", ["pinhole", "lens"])
def test_the_oracle_decodes_every_template_of_library_a(family):
    """the fixture: every template is found with score 1 and its own id in a tilted frame that holds it, under each camera"""
    seen = collections.Counter()
    for r in NS.runs("A", family):
        planted = {m.template for m in r.scene.markers}
        for m in r.ref:
            if m.score == 1 and m.templateId in planted:
                seen[m.templateId] += 1
    print("\n%s: decoded plantings per template %s" % (family, [seen[t] for t in range(16)]))
    assert all(seen[t] >= 1 for t in range(16)), sorted(t for t in range(16) if not seen[t])
    # the frames are what the module says: four different templates each, every template in every quadrant
    sc = NS.scenes(family)
    assert len(sc) == 16 and all(len({m.template for m in s.markers}) == 4 for s in sc)
    assert {(m.template, m.tag) for s in sc for m in s.markers} == {(t, q) for t in range(16) for q in range(4)}
    assert {m.tilt for s in sc for m in s.markers} == set(NS.TILTS)


@pytest.mark.parametrize("which", ["A", "B"])
def test_codes_equal_the_oracles_on_every_candidate(emul, which):
    """emul_read_code through every patch shape of the library, on every square of every frame: the oracle's bit"""
    _, tpls, _ = NS.library(which)
    codes = collections.defaultdict(set)
    n = 0
    for family in NS.FAMILIES:
        for r in NS.runs(which, family):
            quads = H.oracle_find_squares(r.gray)
            for c in r.cands:
                crop, cw, ch = NS.crop_of(r.gray, quads[c.markerId])
                t = tpls[c.templateId]
                pp = np.array(c.patPoint, np.float32)
                bit = emul.emul_read_code(C.c_void_p(crop.ctypes.data), cw, ch, NS.WIDTH, P(pp), t.width, t.height)
                assert bit == c.bit, (which, r.scene.name, c.markerId, c.templateId, (t.width, t.height), bit, c.bit)
                codes[(t.width, t.height)].add(c.bit)
                n += 1
    print("\nlibrary %s: %d candidates; distinct codes per size %s" % (
        which, n, {"%dx%d" % k: len(v) for k, v in codes.items()}))
    assert set(codes) == set(NS.SIZES[which]) and n >= 16 * 36 * 3
    if which == "B":
        for size, seen in codes.items():
            assert len(seen) >= 8, (size, len(seen))


def test_every_64_cell_class_shows_a_negative_code():
    """lane 63 of the device's ballot is the sign bit of the code: each 64-cell class of library B is seen with it set.  (On a
    marker's outer border the cell of lane 63, an end cell of the patch, lies in the black frame; the negative codes come from
    the light blocks of cells that the oracle finds as squares of their own, see nonsquare_scenes.LIBRARY_SEED.)"""
    _, tpls, _ = NS.library("B")
    neg = collections.Counter()
    for family in NS.FAMILIES:
        for r in NS.runs("B", family):
            for c in r.cands:
                t = tpls[c.templateId]
                neg[(t.width, t.height)] += c.bit < 0
    print("\nnegative codes per 64-cell class: %s" % {"%dx%d" % s: neg[s] for s in NS.SIZES_B if s[0] * s[1] == 64})
    for size in NS.SIZES_B:
        if size[0] * size[1] == 64:
            assert neg[size] >= 1, size


def host_against_oracle(emul, run):
    """worst relative difference of the host core's glMatrix to the record's, over the defined records of a run"""
    worst = 0.0
    for m, ok in zip(run.ref, run.defined):
        if not ok:
            continue
        sq = np.array(m.square, np.float32)
        g, ref = np.zeros(16), np.array(m.glMatrix)
        emul.emul_square_to_glmatrix(P(sq), C.byref(run.scene.cam), C.c_double(m.aspectRatio), P(g))
        rel = np.abs(g - ref).max() / max(1.0, np.abs(ref).max())
        assert rel <= HOST_RTOL, (run.scene.name, m.templateId, m.score, rel)
        worst = max(worst, rel)
    return worst


def test_poses_of_tilted_frames_are_all_defined(emul):
    """every record of the 32 tilted frames (the score-0 records of template 0 = 4x2 included) has a pose the reference
    defines, and the host core meets it"""
    n, worst, ratios = 0, 0.0, set()
    for family in ("pinhole", "lens"):
        for r in NS.runs("A", family):
            assert all(r.defined), (r.scene.name, r.movement)
            for m in r.ref:
                w, h = NS.SIZES_A[m.templateId]
                assert m.aspectRatio == w / h
                ratios.add(m.aspectRatio)
            worst = max(worst, host_against_oracle(emul, r))
            n += len(r.ref)
    print("\ntilted frames: %d records, 0 excluded, %d distinct ratios, worst host-to-oracle pose difference %.2g" % (
        n, len(ratios), worst))
    assert n >= 32 and len(ratios) >= 8 and any(m.score == 0 and m.aspectRatio == 2.0
                                                for f in ("pinhole", "lens") for r in NS.runs("A", f) for m in r.ref)


def test_frontal_frames_exclude_what_the_reference_does_not_define(emul):
    n = excluded = 0
    worst = 0.0
    for r in NS.runs("A", "frontal"):
        for m, ok, mv in zip(r.ref, r.defined, r.movement):
            n += 1
            if not ok:
                excluded += 1
                print("\nexcluded: %s template %d score %g, one ulp moves the oracle's pose by %.3g" % (
                    r.scene.name, m.templateId, m.score, mv))
        worst = max(worst, host_against_oracle(emul, r))
    print("\nfrontal frames: %d records, %d excluded, worst host-to-oracle pose difference on the others %.2g" % (
        n, excluded, worst))
    assert excluded >= 1 and 2 * (n - excluded) >= n


def test_pose_is_defined_is_the_ulp_rule():
    cam = NS.camera()
    sq = np.array([200, 150, 330, 160, 320, 290, 190, 280], np.float32)
    assert NS.pose_is_defined(sq, 1.0, cam) and NS.pose_movement(sq, 1.0, cam) > 0
    r = next(r for r in NS.runs("A", "frontal") if not all(r.defined))
    k = r.defined.index(False)
    assert not NS.pose_is_defined(np.array(r.ref[k].square, np.float32), r.ref[k].aspectRatio, r.scene.cam)


def test_template_files_of_every_size(tmp_path):
    """cvarLoadTemplateTag on non-square PNG files against orc_load_template_pixels: width, height and the four codes.

    acBitRotate turns the grid with acArray2DRotateub, whose index formulas are a square grid's: with w != h it reads
    t[(h-1-j)*w+i] for j up to w-1 (index -8 for 4x2), outside the reference's copy of the grid, where the reference reads
    whatever its memory holds.  The host library and the oracle both take such a cell as 0, so every code is below 2^(w*h)
    and the same in every process."""
    import __graft_entry__ as g
    g.build()
    host = C.CDLL(os.path.join(H.PKG, "lib", "libopencv-ar.so.1.0.0"))
    _, tpls, _ = NS.library("A")
    got = NS.templates_from_png(host, tmp_path)
    assert len(got) == 16
    for t, ref, size in zip(got, tpls, NS.SIZES_A):
        assert (t.width, t.height) == (ref.width, ref.height) == size
        assert [int(c) for c in t.code] == [int(c) for c in ref.code], size
        assert t.scale == ref.scale
        assert all((int(c) & (2 ** 64 - 1)) < 2 ** (size[0] * size[1]) for c in t.code), size   # (64 cells: any long long)
    again = H.oracle_templates(NS.library("A")[0])
    assert bytes(again) == bytes(tpls)
