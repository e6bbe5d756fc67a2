"""CPU proof that the scenes of tests/follow_limit_scenes.py reach the follower limits they name, on borders that own a quad.

The parity tests' point-rich borders (the sawtooth frames with teeth of 4 px and more, full-frame noise) never yield a quad:
the adaptive threshold turns a filled shape into an edge band whose teeth no longer approximate to four vertices.  All the GPU
is held to there is that no quad comes out either -- so a tier that dropped or garbled stored points, or a key that lost its
top bits, would pass (test_parity_frames_yield_no_quad_from_a_long_border turns that into a check).  The scenes here are built
from teeth of 2 px and plain squares, whose borders do own quads; this file proves on the oracle and on the host build of the
tiers (tests/emul/follow_emul.cpp), before the GPU is asked anything, that
  * every quad's owning border has exactly the point count, remainder, key branch and vertex-at-seam class the scene names,
    and tier 2's walk of it flushes its points as the scene names: the flush seams are the point counts after every block of
    32 steps of that walk, taken from the host build -- they are no multiples of 32;
  * trace_flat, tier 2, trace_border and tier 3 close that border with as many corner points as the oracle's contour has;
  * the quad depends on the points at the seams.

What the sensitivity test means for tests/test_gpu_follow_limits.py, which compares quads only: at every seam index of every
owning border, a point replaced by (0, 0) changes orc_approx_poly's output -- a point that was not written, or a stale value
in its place, is noticed anywhere.  Removing a point changes the output where the point is a quad vertex (the vertex-at-seam
scenes), so a dropped point, or points shifted by one, are noticed only at a vertex.  Two neighbouring points swapped are not
noticed: the approximation keeps the same four vertices.
"""
import numpy as np
import pytest

import follow_limit_scenes as S
from test_follow_tiers_cpu import OK, check_walks, lib   # noqa: F401  (lib: the fixture that builds tests/emul/follow_emul.cpp)
from test_starts_cpu import build_lib

_analysed = {}


def analysed(scene):
    """the oracle's analysis of a scene, computed once"""
    if scene.name not in _analysed:
        _analysed[scene.name] = S.analyse(scene.make())
    return _analysed[scene.name]


def reached(lib, a, o):   # noqa: F811
    return S.classes_of(o) | S.tier2_classes(o, S.tier2_marks(lib, a.binary, o))


def match_groups(scene, a, lib):   # noqa: F811
    """the owning border of every class group of the scene: each owner takes one group"""
    assert len(a.quads) == len(a.owners) == len(scene.classes), (scene.name, len(a.quads), [o.n for o in a.owners])
    assert len({o.contour for o in a.owners}) == len(a.owners), (scene.name, "two quads of one border")
    left = list(a.owners)
    out = []
    for group in scene.classes:
        hit = [o for o in left if set(group) <= reached(lib, a, o)]
        assert len(hit) == 1, (scene.name, group, [sorted(reached(lib, a, o)) for o in left])
        left.remove(hit[0])
        out.append(hit[0])
    return out


BY_NAME = {s.name: s for s in S.SCENES}


@pytest.mark.parametrize("name", list(BY_NAME))
def test_scene_reaches_the_classes_it_names(lib, name):   # noqa: F811
    scene = BY_NAME[name]
    a = analysed(scene)
    owners = match_groups(scene, a, lib)
    for o in owners:
        # the owner is the border the quad comes from, and each vertex is one point of it
        assert np.array_equal(S.approx(a.contours[o.contour]), a.quads[o.quad]), (name, o)
        assert all(len(v) == 1 for v in o.vertex_index), (name, o)
    print(name, [(o.n, o.n % 64, S.key_branch(o), o.diag2, [v[0] for v in o.vertex_index], sorted(S.tier2_classes(o, S.tier2_marks(lib, a.binary, o))))
                 for o in owners])


def test_the_scenes_cover_the_required_classes():
    reached = set()
    for s in S.SCENES:
        for group in s.classes:
            reached |= set(group)
    # both sides of the lane slab / LDS staging / key count limit, and of the wave slab
    for n in (S.SLAB_PTS - 1, S.SLAB_PTS, S.SLAB_PTS + 1, S.SLAB3_PTS - 1, S.SLAB3_PTS, S.SLAB3_PTS + 1):
        assert "n=%d" % n in reached, n
    # last store of tier 3: 63, 0 and 1 points, either side of the wave slab's end
    for n, r64 in ((8191, 63), (8192, 0), (8193, 1)):
        assert any({"n=%d" % n, "n%%64=%d" % r64} <= set(g) for s in S.SCENES for g in s.classes), n
    # tier 2's flushes: a walk that closes with nothing, one point and more left to flush; a full row of 32; the slab exactly
    # full; the block that crosses the slab's end cut short; a vertex either side of a flush seam
    assert {"t2last=0", "t2last=1", "t2full", "vertex@t2flush"} <= reached
    assert any({"n=%d" % S.SLAB_PTS} <= set(g) and any(c.startswith("t2last=") and c != "t2last=0" for c in g) for s in S.SCENES for g in s.classes)
    assert any({"n=%d" % (S.SLAB_PTS + 1)} <= set(g) and any(c.startswith("t2cut=") for c in g) for s in S.SCENES for g in s.classes)
    # the key width: the box at its limit from both sides, each term of the condition deciding alone
    assert any({"key32", "diag2=%d" % ((1 << 21) - 4094)} <= set(g) for s in S.SCENES for g in s.classes)
    assert any({"key64:box", "diag2=%d" % (1 << 21)} <= set(g) for s in S.SCENES for g in s.classes)
    assert sum("key64:box" in g for s in S.SCENES for g in s.classes) >= 2 and "key64:n" in reached
    # a vertex at every kind of seam but the one listed as left out
    assert len(S.SEAMS_LEFT_OUT) <= 1
    assert {k for k in S.SEAMS if k in reached} == set(S.SEAMS) - set(S.SEAMS_LEFT_OUT)
    # only duplicates are kept from the full pipeline
    for s in S.SCENES:
        if s.seam_only:
            assert any("vertex@" in c for g in s.classes for c in g), s.name


@pytest.mark.parametrize("name", list(BY_NAME))
def test_walk_data_of_the_owning_borders(lib, name):   # noqa: F811
    scene = BY_NAME[name]
    a = analysed(scene)
    rows = S.walk_rows(lib, a.binary)
    check_walks(rows, name)   # all four forms agree on every plausible start of the plane
    steps = []   # (points, tier 2's step count) of the owning borders: what tier 2's budget is placed by
    for o in a.owners:
        r = S.owner_row(rows, o, a.binary.shape[1])
        assert r[2] == OK and r[5] == OK and r[9] == OK and r[12] == OK, (name, o, r.tolist())
        assert r[3] == r[6] == r[10] == r[13] == o.n == len(a.contours[o.contour]), (name, o, r.tolist())
        assert r[8] == 1 and r[15] == 1
        assert len(S.tier2_marks(lib, a.binary, o)) == S.tier2_blocks(r[7])   # (one flush per block of that walk)
        steps.append((o.n, int(r[7])))
    print(name, "points, steps:", steps)


@pytest.mark.parametrize("name", list(BY_NAME))
def test_quads_depend_on_the_points_at_the_seams(lib, name):   # noqa: F811
    scene = BY_NAME[name]
    a = analysed(scene)
    for o in a.owners:
        pts = a.contours[o.contour]
        seams = S.seam_indices(o.n, S.tier2_marks(lib, a.binary, o))
        assert o.n - 1 in seams or o.n not in (S.SLAB_PTS, S.SLAB3_PTS)   # (the last slot of a slab exactly full)
        for i in seams:
            mut = pts.copy()
            mut[i] = 0
            assert not np.array_equal(S.approx(mut), a.quads[o.quad]), (name, o.n, i)
        # a vertex at a seam: without that point the quad is another one
        for (idx,) in o.vertex_index:
            if idx in seams:
                assert not np.array_equal(S.approx(np.delete(pts, idx, axis=0)), a.quads[o.quad]), (name, o.n, idx)


@pytest.mark.parametrize("name", [s.name for s in S.SCENES if (s.w, s.h) == (640, 480)])
def test_only_the_frames_own_border_skips_tier_2(lib, name):   # noqa: F811
    """with mid_steps as large as it goes every border closes in tier 2 but those tier 1 sends straight to tier 3: in the
    640x480 scenes the frame's own border, found at (1, 1), four points -- never an owning border"""
    a = analysed(BY_NAME[name])
    ns = (a.binary.shape[1] + 15) & ~15
    straight = S.straight_starts(lib, build_lib(), a.binary)
    assert straight[:, :2].tolist() == [[ns + 1, 0]], (name, straight.tolist())
    assert all(o.start != (1, 1) for o in a.owners)


def test_the_budget_case_exists(lib):   # noqa: F811
    """what test_gpu_follow_limits.py's budget test counts: of the starts handed to the followers, those whose walk ends in the
    owning border's own block of steps are closed borders (here: the owning border alone)"""
    scene, lo, hi, n = S.budget_case(lib, build_lib())
    assert hi == lo + S.MID_BLOCK and n >= 1
    a = analysed(scene)
    steps = [int(S.owner_row(S.walk_rows(lib, a.binary), o, a.binary.shape[1])[7]) for o in a.owners]
    assert any(lo < t <= hi for t in steps), (scene.name, lo, hi, steps)
    print(scene.name, lo, hi, n)


# largest border (corner points) of the parity tests' frames
LONGEST = {"thousands_0": 26, "thousands_1": 3509, "capacity": 10229, "noise": 12699}


def test_parity_frames_yield_no_quad_from_a_long_border():
    """the reason for this file: in tests/test_gpu_parity.py no border of more than 1024 points owns a quad"""
    for name, frame in S.parity_frames().items():
        a = S.analyse(frame, min_pts=S.SLAB_PTS + 1)
        assert max(len(c) for c in a.contours) == LONGEST[name], (name, max(len(c) for c in a.contours))
        assert a.owners == [], (name, [o.n for o in a.owners])
    # the frame that test_borders_with_thousands_of_points gains does
    a = S.analyse(S.thousands_tooth2(), min_pts=S.SLAB_PTS + 1)
    assert sorted(o.n for o in a.owners) == [2012, 2974] and len(a.quads) == 2
