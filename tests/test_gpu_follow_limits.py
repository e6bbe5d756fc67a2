"""GPU tests of the follower's slab, pool and key-width limits on borders that own a quad (tests/follow_limit_scenes.py; what
each scene reaches is proved on the CPU by tests/test_follow_limits_cpu.py, which also says what a comparison of quads notices
and what it does not).

Code that only the GPU compiles, and what reaches it here:
  * tier 2's parking of corner points in LDS and their flush to the lane slabs after every block of MID_BLOCK = 32 steps: full
    rows of 32 points (the rhombi), a last flush of 0, 1 and 3 .. 18 points, a quad vertex either side of a flush seam, the
    slab exactly full (1024), the block that crosses its end cut short and the overflow path follow_overflow beyond it (1025,
    1026) -- the flush sizes and seams are those of the border's own walk, derived on the CPU: every scene with mid_steps as
    large as the setter takes, so that every border closes in tier 2;
  * tier 3's parking of points in lanes and their 64-at-a-time store into the wave slab, a last store of 63, 0 and 1 points,
    the slab exactly full (8192) and the second follow into the pool beyond it (8193): every scene with mid_steps = 64, so
    that every long border goes to tier 3;
  * wave_finish_packed staged (n <= 1024) and unstaged, from a lane slab, a wave slab and the pool;
  * wave_approx_dp with 32-bit keys up to n = 1024 and a squared diagonal of 2^21 - 4094, with 64-bit keys from n = 1025 or a
    squared diagonal of exactly 2^21.
Every scene must give the oracle's quads -- count, order, every integer -- under the defaults and both settings, and the work
counters (ocvar_hip_counters: 5 ints taken from the point pool, 8 / 9 starts handed to tier 3 by the frame / crop pass) must
show that the intended path was taken."""
from types import SimpleNamespace

import numpy as np
import pytest

import follow_limit_scenes as S
from frame_kit import oa  # noqa: F401
from test_follow_tiers_cpu import lib   # noqa: F401  (lib: the fixture that builds tests/emul/follow_emul.cpp)
from test_gpu_parity import OracleFrame, check_candidates, check_markers, check_planes, make_detector
from test_starts_cpu import build_lib

pytestmark = pytest.mark.gpu

POOL, LONG_F, LONG_C = 5, 8, 9   # ocvar_hip_counters
# ocvar_hip_set_tuning; 0 restores a default.  "tier3" is the setting test_crop_pass_one_and_two_phases_give_the_same_results uses.
SETTINGS = {"defaults": dict(mid_steps=0, mid_blocks=0, long_blocks=0),
            "tier2": dict(mid_steps=2 ** 31 - 1, mid_blocks=0, long_blocks=0),
            "tier3": dict(mid_steps=64, mid_blocks=3, long_blocks=2)}
BY_NAME = {s.name: s for s in S.SCENES}


@pytest.fixture(scope="module")
def contexts(oa):
    """one context per frame size (max_batch 1), created once for the module"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = make_detector(oa, SimpleNamespace(width=w, height=h), ["2x2-01"], 1)
        return made[(w, h)]
    yield get
    for det, _, _ in made.values():
        det.close()


_refs = {}


def reference(scene, tpls=None, cam=None):
    """the frame, the oracle's analysis and -- when templates and camera are given -- its full results, computed once per scene"""
    if scene.name not in _refs:
        frame = scene.make()
        _refs[scene.name] = [frame, S.analyse(frame), None]
    r = _refs[scene.name]
    if tpls is not None and r[2] is None:
        r[2] = OracleFrame(r[0], tpls, cam)
    return r


def closed_borders_over(a, limit):
    """point counts of the frame's borders with more than `limit` points that the finishing code approximates (bounding box
    area > 500: worth_approximating)"""
    return [len(c) for c in a.contours if len(c) > limit and
            int(c[:, 0].max() - c[:, 0].min()) * int(c[:, 1].max() - c[:, 1].min()) > 500]


def check_counters(scene, setting, a, c, straight):
    """The frame pass's counters after find_squares.  straight: the starts tier 1 sends to tier 3 itself, whatever tier 2's
    budget (S.straight_starts, which restates route 2 of follow.hip::follow_short) -- in the 640x480 scenes the frame's own four-point border and nothing else, which
    test_follow_limits_cpu.py::test_only_the_frames_own_border_skips_tier_2 proves; apart from it nothing may reach tier 3
    when tier 2's budget has no end."""
    over_slab, over_slab3 = closed_borders_over(a, S.SLAB_PTS), closed_borders_over(a, S.SLAB3_PTS)
    what = (scene.name, setting, c.tolist(), over_slab)
    if setting == "tier2":
        if (scene.w, scene.h) == (640, 480):
            assert len(straight) == 1 and c[LONG_F] - len(straight) == 0, what   # every other border closed in tier 2
        # follow_overflow takes 2 n ints for the points and 2 (n + 2) for the approximation's stack, once per border beyond the slab
        assert c[POOL] == sum(2 * n + 2 * (n + 2) for n in over_slab), what
    if setting == "tier3":
        assert c[LONG_F] >= len(a.owners), what
        # the second follow of a border with more points than the wave slab holds takes n + 64 ints
        assert c[POOL] == sum(n + 64 for n in over_slab3), what


@pytest.fixture(scope="module")
def starts_lib():
    return build_lib()


@pytest.mark.parametrize("name", list(BY_NAME))
def test_frame_pass_quads_equal_the_oracle_in_every_tier(contexts, lib, starts_lib, name):   # noqa: F811
    scene = BY_NAME[name]
    det, _, _ = contexts(scene.w, scene.h)
    _, a, _ = reference(scene)
    assert len(a.quads) == len(scene.classes)
    straight = S.straight_starts(lib, starts_lib, a.binary) if (scene.w, scene.h) == (640, 480) else None
    for setting, knobs in SETTINGS.items():
        det.set_tuning(**knobs)
        got, n = det.find_squares(a.gray)
        c = det.counters()
        print(name, setting, "counters", c.tolist())
        assert n == len(a.quads) and np.array_equal(got, a.quads), (name, setting, n, got.tolist(), a.quads.tolist())
        check_counters(scene, setting, a, c, straight)
    det.set_tuning(**SETTINGS["defaults"])


@pytest.mark.parametrize("name", [s.name for s in S.SCENES if not s.seam_only])
def test_full_pipeline_equals_the_oracle_in_every_tier(contexts, name):
    """detect_host: planes, frame quads, candidates -- and with them the crop pass's quads -- and markers, as
    test_gpu_parity.check_frame compares them (its three checks, on a reference computed once)"""
    scene = BY_NAME[name]
    det, tpls, cam = contexts(scene.w, scene.h)
    frame, a, ref = reference(scene, tpls, cam)
    results = {}
    for setting, knobs in SETTINGS.items():
        det.set_tuning(**knobs)
        markers, counts = det.detect_host(frame[None].copy())
        c = det.counters()
        print(name, setting, "counters", c.tolist())
        check_planes(det, 0, ref, (name, setting))
        check_candidates(det, 0, ref, (name, setting))
        check_markers(0, ref, markers, counts, (name, setting))
        results[setting] = (markers.tobytes(), counts.tobytes())
        if setting == "tier3":
            assert c[LONG_F] >= len(a.owners), (name, c.tolist())
            # the crops of the frame's quads hold the same borders again: walks of more than 64 steps, so tier 3 is used
            if name == S.SCENES[0].name:
                assert c[LONG_C] > 0, (name, c.tolist())
    det.set_tuning(**SETTINGS["defaults"])
    assert len(a.quads) >= 2 and len(ref.cands) >= 1   # (a crop's quad reached the decoder: check_candidates compared it)
    assert results["defaults"] == results["tier2"] == results["tier3"], name


def test_tier_2_budget_decides_where_the_owning_border_closes(contexts, lib, starts_lib):   # noqa: F811
    """mid_steps one block of 32 steps short of the owning border's walk, then the block that covers it: the starts handed to
    tier 3 differ by the walks that end in that block (counted on the CPU from fe_walks); the quads do not change"""
    scene, lo, hi, n_between = S.budget_case(lib, starts_lib)
    det, _, _ = contexts(scene.w, scene.h)
    _, a, _ = reference(scene)
    handed = {}
    for budget in (lo, hi):
        det.set_tuning(mid_steps=budget, mid_blocks=0, long_blocks=0)
        got, n = det.find_squares(a.gray)
        handed[budget] = int(det.counters()[LONG_F])
        assert n == len(a.quads) and np.array_equal(got, a.quads), (scene.name, budget)
    det.set_tuning(**SETTINGS["defaults"])
    print(scene.name, lo, hi, handed, n_between)
    assert handed[lo] - handed[hi] == n_between >= 1, (scene.name, lo, hi, handed, n_between)
