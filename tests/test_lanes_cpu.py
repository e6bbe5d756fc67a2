"""CPU tests of the gate's scheduling policy (opencv-ar_amd/csrc/lanes_core.h, built for the host from tests/emul/lanes_emul.cpp)
on a simulated timeline: lanes are queues that run their entries in order, a gated segment starts when the launch its ticket
names has finished, and the host collects and re-enqueues as bench.py does -- or in a random order."""
import ctypes as C

import numpy as np
import pytest

from hostbuild import host_core


@pytest.fixture(scope="module")
def lib():
    L = host_core("lanes_emul")
    vp, i = C.c_void_p, C.c_int
    L.lanes_emul_init.argtypes = [vp, i, i]
    L.lanes_emul_choose.argtypes = [vp]
    L.lanes_emul_book.argtypes = [vp, i]
    L.lanes_emul_retire.argtypes = [vp, i]
    L.lanes_emul_outstanding.argtypes = [vp, i]
    L.lanes_emul_ticket.argtypes = [vp]
    L.lanes_emul_ticket.restype = C.c_longlong
    L.lanes_emul_wait_for.argtypes = [vp]
    L.lanes_emul_wait_for.restype = C.c_longlong
    L.lanes_emul_refresh.argtypes = [vp, vp, i, vp]
    L.lanes_emul_place.argtypes = [vp, vp, i, vp]
    L.lanes_emul_for_queues.argtypes = [i, i]
    L.lanes_emul_parse.argtypes = [C.c_char_p]
    return L


class Sim:
    """The device side of a gate: every lane runs its segments in order.  A batch is four segments -- frame binarise (gated),
    followers, crop binarise (gated), the rest -- of given lengths; a gated segment starts when the segment in front of it in
    its lane has ended AND the gated segment its ticket waits for has ended.  The host side is gate.hip's: one batch in flight
    per context, placed by lane_place, whose "finished" callback reads the simulated clock."""

    def __init__(self, L, n_lanes, width, n_ctx):
        self.L, self.n_lanes, self.width, self.n_ctx = L, n_lanes, width, n_ctx
        self.s = C.create_string_buffer(L.lanes_emul_sizeof())
        L.lanes_emul_init(self.s, n_lanes, width)
        self.lanes = [[] for _ in range(n_lanes)]   # per lane: segments in submission order
        self.ticket_seg = {}                        # ticket -> segment
        self.lane_of = (C.c_int * n_ctx)(*([-1] * n_ctx))   # per context: the lane that still counts its batch
        self.last_seg = [None] * n_ctx                       # per context: the last segment of its batch in flight
        self.retired_early = 0
        self.now = 0.0

    def outstanding(self):
        return [self.L.lanes_emul_outstanding(self.s, l) for l in range(self.n_lanes)]

    def done_table(self):
        assert self.settle(), "a submitted segment can never start: deadlock"
        return (C.c_int * self.n_ctx)(*[int(seg is not None and seg["end"] <= self.now) for seg in self.last_seg])

    def enqueue(self, ctx, lengths):
        """places a batch of context ctx as gate.hip does; returns (lane, lanes' outstanding work at the placement)"""
        assert self.lane_of[ctx] == -1
        # (the two halves of lane_place apart, to see the counts it chose from; test_place_is_refresh_choose_book ties them)
        counted = sum(1 for l in self.lane_of if l >= 0)
        self.L.lanes_emul_refresh(self.s, self.lane_of, self.n_ctx, self.done_table())
        self.retired_early += counted - sum(1 for l in self.lane_of if l >= 0)
        before = self.outstanding()
        assert sum(before) == sum(1 for l in self.lane_of if l >= 0)
        lane = self.L.lanes_emul_choose(self.s)
        self.L.lanes_emul_book(self.s, lane)
        self.lane_of[ctx] = lane
        for k, d in enumerate(lengths):
            seg = {"len": float(d), "gated": k in (0, 2), "wait": None, "start": None, "end": None, "submitted": self.now}
            if seg["gated"]:
                w = self.L.lanes_emul_wait_for(self.s)
                n = self.L.lanes_emul_ticket(self.s)
                assert w == (n - self.width if n >= self.width else -1)
                seg["wait"] = self.ticket_seg[w] if w >= 0 else None
                self.ticket_seg[n] = seg
            self.lanes[lane].append(seg)
        self.last_seg[ctx] = self.lanes[lane][-1]
        return lane, before

    def collect(self, ctx):
        """the host waits for the context's batch: time moves to its end"""
        assert self.settle(), "a submitted segment can never start: deadlock"
        self.now = max(self.now, self.last_seg[ctx]["end"])
        if self.lane_of[ctx] >= 0:   # (else: a placement has seen it finished already)
            self.L.lanes_emul_retire(self.s, self.lane_of[ctx])
            self.lane_of[ctx] = -1
        self.last_seg[ctx] = None

    def settle(self):
        """start and end times of every segment that can be given one; returns False if nothing is left without"""
        changed = True
        while changed:
            changed = False
            for segs in self.lanes:
                prev_end = 0.0
                for seg in segs:
                    if seg["end"] is None:
                        if prev_end is None or (seg["wait"] is not None and seg["wait"]["end"] is None):
                            break
                        seg["start"] = max(prev_end, seg["submitted"], seg["wait"]["end"] if seg["wait"] else 0.0)
                        seg["end"] = seg["start"] + seg["len"]
                        changed = True
                    prev_end = seg["end"]
        return all(seg["end"] is not None for segs in self.lanes for seg in segs)

    def max_gated_at_once(self):
        ev = []
        for segs in self.lanes:
            for seg in segs:
                if seg["gated"]:
                    ev += [(seg["start"], 1), (seg["end"], -1)]
        ev.sort(key=lambda e: (e[0], e[1]))   # (an end before a start at the same instant)
        run = peak = 0
        for _, d in ev:
            run += d
            peak = max(peak, run)
        return peak


@pytest.mark.parametrize("seed", range(40))
def test_policy_on_a_simulated_timeline(lib, seed):
    """random chain lengths, 1 - 8 contexts, 1 - 8 lanes, widths 1 - 3; host order as bench.py's (round robin) or random:
    never more than `width` gated segments running, every batch completes, every batch lands on a lane whose outstanding work
    -- batches neither collected nor finished by the simulated clock -- was minimal, and the lanes' counts differ by at most
    one after a placement that found them so."""
    rng = np.random.default_rng(seed)
    n_ctx, n_lanes, width = int(rng.integers(1, 9)), int(rng.integers(1, 9)), int(rng.integers(1, 4))
    sim = Sim(lib, n_lanes, width, n_ctx)
    in_flight = set()
    steps = 12
    left = {c: steps for c in range(n_ctx)}
    done = 0

    def enqueue(c):
        lane, before = sim.enqueue(c, rng.uniform(0.1, 5.0, size=4) * rng.choice([1.0, 1.0, 8.0]))
        assert before[lane] == min(before), (before, lane)
        after = sim.outstanding()
        assert sum(after) == sum(before) + 1
        if max(before) - min(before) <= 1:
            assert max(after) - min(after) <= 1, (before, after)
        in_flight.add(c)
        left[c] -= 1

    for c in range(n_ctx):
        enqueue(c)
    round_robin = seed % 2 == 0
    k = 0
    while in_flight:
        c = sorted(in_flight)[k % len(in_flight)] if round_robin else int(rng.choice(sorted(in_flight)))
        k += 1
        sim.collect(c)
        in_flight.discard(c)
        done += 1
        if left[c] > 0:
            enqueue(c)
    assert done == n_ctx * steps
    assert sim.settle()
    assert sim.outstanding() == [0] * n_lanes
    assert 1 <= sim.max_gated_at_once() <= width
    # every lane ran its segments in order, and no segment before it was submitted
    for segs in sim.lanes:
        for a, b in zip(segs, segs[1:]):
            assert b["start"] >= a["end"]
        assert all(seg["start"] >= seg["submitted"] for seg in segs)


def test_finished_batches_do_not_count_at_a_placement(lib):
    """two lanes, three contexts: context 0's short batch has finished (by the clock) when context 2 is collected and
    re-enqueued, though nobody has collected it -- its lane counts as empty and takes the batch; without the refresh the other
    lane would have been the tie's choice"""
    sim = Sim(lib, 2, 3, 3)
    assert sim.enqueue(0, [1, 1, 1, 1])[0] == 0
    assert sim.enqueue(1, [1, 50, 1, 1])[0] == 1       # (its long segment is not a gated one: nobody waits for it at the gate)
    assert sim.enqueue(2, [1, 1, 1, 1])[0] == 0       # behind context 0's
    sim.collect(2)                                     # the clock is at 8: context 0's batch ended at 4, context 1's runs until 53
    lane, before = sim.enqueue(2, [1, 1, 1, 1])
    assert before == [0, 1] and lane == 0 and sim.retired_early == 1
    assert sim.lane_of[0] == -1
    sim.collect(0)                                     # collecting it later retires nothing twice
    assert sim.outstanding() == [1, 1]
    sim.collect(1)
    sim.collect(2)
    assert sim.outstanding() == [0, 0]


def test_place_is_refresh_choose_book(lib):
    """lane_place (what gate.hip calls) against its three steps on a copy of the same state"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        n_lanes, n = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        a, b = (C.create_string_buffer(lib.lanes_emul_sizeof()) for _ in range(2))
        lanes = [int(rng.integers(-1, n_lanes)) for _ in range(n)]
        for s in (a, b):
            lib.lanes_emul_init(s, n_lanes, 2)
            for l in lanes:
                if l >= 0:
                    lib.lanes_emul_book(s, l)
        done = (C.c_int * n)(*[int(rng.integers(0, 2)) for _ in range(n)])
        la, lb = (C.c_int * n)(*lanes), (C.c_int * n)(*lanes)
        got = lib.lanes_emul_place(a, la, n, done)
        lib.lanes_emul_refresh(b, lb, n, done)
        want = lib.lanes_emul_choose(b)
        lib.lanes_emul_book(b, want)
        assert got == want and list(la) == list(lb)
        assert [lib.lanes_emul_outstanding(a, l) for l in range(n_lanes)] == [lib.lanes_emul_outstanding(b, l) for l in range(n_lanes)]
        assert all(la[i] == (-1 if done[i] else lanes[i]) for i in range(n))


def test_the_doubled_up_lane_rotates(lib):
    """five contexts on three lanes in bench.py's order: the two contexts that share a lane are not the same pair for ever"""
    sim = Sim(lib, 3, 2, 5)
    lane_of = {}
    pairs = set()
    for c in range(5):
        lane_of[c] = sim.enqueue(c, [1, 1, 1, 1])[0]
    for step in range(12):
        for c in range(5):
            sim.collect(c)
            lane_of[c] = sim.enqueue(c, [1, 1, 1, 1])[0]
            by_lane = {}
            for cc, l in lane_of.items():
                by_lane.setdefault(l, []).append(cc)
            assert sorted(len(v) for v in by_lane.values()) == [1, 2, 2]
            pairs |= {tuple(sorted(v)) for v in by_lane.values() if len(v) == 2}
    assert len(pairs) > 2


def test_lane_count_from_the_queue_count(lib):
    f = lib.lanes_emul_for_queues
    assert f(0, 0) == 4 and f(4, 0) == 4          # the runtime's default of four queues
    assert f(8, 0) == 8 and f(32, 0) == lib.lanes_emul_max() == 8
    assert f(1, 0) == 1 and f(2, 0) == 2
    assert [f(4, k) for k in (1, 2, 4, 8, 99)] == [1, 2, 4, 8, 8]
    p = lib.lanes_emul_parse
    assert p(None) == 0 and p(b"") == 0 and p(b"4") == 4 and p(b"32") == 32 and p(b"x") == 0 and p(b"-1") == 0 and p(b"4 ") == 0
