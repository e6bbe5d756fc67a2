"""CPU tests of the template-library cores (opencv-ar_amd/csrc/library_core.h, the sparse elimination of tail_core.h), built
for the host from tests/emul/library_emul.cpp: the code lookup against the reference's linear match_orient, the orient 2/4
rotation as a prefix shift against sequential rot_square, and the sparse survivors against the literal `||` loop."""
import ctypes as C
import itertools

import numpy as np
import pytest

import helpers as H
from helpers import P
from hostbuild import host_core


@pytest.fixture(scope="module")
def lib():
    L = host_core("library_emul")
    L.lib_set.argtypes = [C.c_void_p, C.c_int]
    L.lib_square_matches.argtypes = [C.c_void_p, C.c_void_p]
    L.lib_candidate_square.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.linear_candidates.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dedupe_agrees.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]
    return L


def rotations(grid):
    """codes of a w x h grid read as acArray2DToBit does (row-major, first cell in the top bit) in its 4 rotations; a
    stand-in for the library's codes: the cores only compare them"""
    out = []
    g = np.asarray(grid)
    for k in range(4):
        r = np.rot90(g, k)
        v = 0
        for b in r.flatten():
            v = (v << 1) | int(b)
        out.append(v - (1 << 64) if v >= 1 << 63 else v)
    return out


def random_library(rng, n, sizes, dup_frac=0.0, sym_frac=0.0):
    """n templates over the given (w, h) sizes; some repeat an earlier template, some have rotationally symmetric codes"""
    arr = (H.Template * n)()
    for i in range(n):
        if i and rng.random() < dup_frac:
            arr[i] = arr[int(rng.integers(0, i))]
            continue
        w, h = sizes[int(rng.integers(0, len(sizes)))]
        if w == h and rng.random() < sym_frac:
            q = rng.integers(0, 2, (w + 1) // 2 * ((h + 1) // 2))
            g = np.zeros((h, w), np.int64)
            half = (w + 1) // 2
            g[:half, :half] = q.reshape(half, half)
            for _ in range(3):   # 4-fold symmetric grid
                g = np.maximum(g, np.rot90(g))
            codes = rotations(g)
        elif w == h:
            codes = rotations(rng.integers(0, 2, (h, w)))
        else:   # non-square codes: any four values (the reference reads what the file gives)
            codes = [int(x) for x in rng.integers(-(1 << 62), 1 << 62, 4)]
            if rng.random() < 0.3:
                codes[2] = codes[0]
        arr[i].width, arr[i].height, arr[i].scale = w, h, 0.01
        for k in range(4):
            arr[i].code[k] = codes[k]
    return arr


def library_arrays(lib, n):
    info = np.zeros(3, np.int32)
    lib.lib_info(P(info))
    n_sizes, n_groups, max_match = (int(x) for x in info)
    group_of, size_of, members = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    group_off = np.zeros(n_groups + 1, np.int32)
    lib.lib_groups(P(group_of), P(size_of), P(group_off), P(members))
    sizes = []
    for s in range(n_sizes):
        wh = np.zeros(2, np.int32)
        lib.lib_size(s, P(wh))
        sizes.append(tuple(int(x) for x in wh))
    return dict(n_sizes=n_sizes, n_groups=n_groups, max_match=max_match, group_of=group_of, size_of=size_of,
                group_off=group_off, members=members, sizes=sizes)


def square_codes(rng, tpls, A):
    """one code per size class: mostly a code of some template of that size (so that there are matches), sometimes noise"""
    codes = np.zeros(A["n_sizes"], np.int64)
    for s in range(A["n_sizes"]):
        ids = np.flatnonzero(A["size_of"] == s)
        if rng.random() < 0.8:
            t = tpls[int(rng.choice(ids))]
            codes[s] = t.code[int(rng.integers(0, 4))]
        else:
            codes[s] = int(rng.integers(-(1 << 62), 1 << 62))
    return codes


def check_library(lib, rng, tpls, trials):
    n = len(tpls)
    assert lib.lib_set(tpls, n) == 0
    A = library_arrays(lib, n)
    assert [A["sizes"][s] for s in A["size_of"]] == [(t.width, t.height) for t in tpls]
    assert all((A["group_of"][A["members"][A["group_off"][g]:A["group_off"][g + 1]]] == g).all() for g in range(A["n_groups"]))
    firsts = A["members"][A["group_off"][:-1]]
    assert (np.diff(firsts) > 0).all(), "groups are numbered in the order of their first members"
    sq = np.array([10.5, 20.25, 90.0, 22.0, 88.5, 101.0, 12.0, 97.75], np.float32)
    for _ in range(trials):
        codes = square_codes(rng, tpls, A)
        m = np.zeros(max(A["max_match"], 1), np.int32)
        nm = lib.lib_square_matches(P(codes), P(m))
        assert nm <= A["max_match"]
        m = m[:nm]
        assert (np.diff(m) > 0).all()
        per_t = codes[A["size_of"]].astype(np.int64)
        orient = np.zeros(n, np.int32)
        lin = np.zeros((n, 8), np.float32)
        lib.linear_candidates(tpls, n, P(per_t), P(sq), P(orient), P(lin))
        # the table's matches, expanded to templates, are match_orient's
        from_table = np.zeros(n, np.int32)
        for x in m:
            g, o = x >> 2, (x & 3) + 1
            from_table[A["members"][A["group_off"][g]:A["group_off"][g + 1]]] = o
        assert np.array_equal(from_table, orient)
        # every candidate's corners: the prefix shift equals the reference's sequential rotations, bit for bit
        for t in sorted(set(rng.integers(0, n, 24).tolist()) | {0, n - 1}):
            out = np.zeros(8, np.float32)
            lib.lib_candidate_square(P(sq), P(m), nm, t, P(out))
            assert np.array_equal(out, lin[t]), t


def test_lookup_and_rotation_prefix_single_size(lib):
    rng = np.random.default_rng(11)
    for n in (1, 3, 17, 256, 4096):
        check_library(lib, rng, random_library(rng, n, [(8, 8)]), 40)


def test_lookup_and_rotation_prefix_duplicates_and_symmetric_codes(lib):
    rng = np.random.default_rng(12)
    for n in (5, 64, 1024):
        check_library(lib, rng, random_library(rng, n, [(4, 4), (6, 6)], dup_frac=0.4, sym_frac=0.3), 60)
    # a library of one template repeated: one group, one match per square at most
    one = random_library(rng, 1, [(8, 8)])
    arr = (H.Template * 4096)(*([one[0]] * 4096))
    assert lib.lib_set(arr, 4096) == 0
    assert library_arrays(lib, 4096)["n_groups"] == 1 and library_arrays(lib, 4096)["max_match"] == 1
    check_library(lib, rng, arr, 10)


def test_lookup_and_rotation_prefix_mixed_sizes(lib):
    rng = np.random.default_rng(13)
    sizes = [(w, w) for w in range(2, 9)] + [(8, 4), (3, 5), (1, 1), (16, 4), (64, 1)]
    for n in (12, 300, 2000):
        check_library(lib, rng, random_library(rng, n, sizes, dup_frac=0.2, sym_frac=0.2), 60)


def test_more_than_16_sizes_is_refused(lib):
    rng = np.random.default_rng(14)
    sizes16 = [(w, h) for w in range(1, 9) for h in (1, 2)]
    assert lib.lib_set(random_library(rng, 64, sizes16), 64) == 0
    t = random_library(rng, 17, [(1, 1)])
    for i, (w, h) in enumerate(sizes16 + [(3, 3)]):
        t[i].width, t[i].height = w, h
    assert lib.lib_set(t, 17) == -1


def agrees(lib, n_match, match, stride, K, n_groups, group_of, group_off, members):
    out = np.zeros(2, np.int32)
    ok = lib.dedupe_agrees(len(n_match), K, P(n_match), P(match), stride, n_groups, P(group_of), P(group_off), P(members),
                           P(out))
    return ok, out


def test_sparse_elimination_equals_literal_loop_exhaustive(lib):
    """every score pattern of up to 4 valid squares x 4 templates (each template its own group)"""
    count = 0
    for K in range(1, 5):
        group_of = np.arange(K, dtype=np.int32)
        group_off = np.arange(K + 1, dtype=np.int32)
        members = np.arange(K, dtype=np.int32)
        for ns in range(1, 5):
            for bits in itertools.product((0, 1), repeat=ns * K):
                S = np.array(bits, np.int32).reshape(ns, K)
                n_match = S.sum(1).astype(np.int32)
                match = np.zeros((ns, K), np.int32)
                for i in range(ns):
                    ts = np.flatnonzero(S[i])
                    match[i, :len(ts)] = ts << 2
                ok, out = agrees(lib, n_match, match, K, K, K, group_of, group_off, members)
                assert ok, (S.tolist(), out.tolist())
                count += 1
    assert count == sum(2 ** (ns * K) for K in range(1, 5) for ns in range(1, 5))


@pytest.mark.parametrize("n_sq,K,density", [(64, 4096, "sparse"), (16, 4096, "dense"), (64, 256, "dense"), (64, 1024, "dup"),
                                            (40, 64, "sparse"), (64, 16, "dense")])
def test_sparse_elimination_equals_literal_loop_random(lib, n_sq, K, density):
    rng = np.random.default_rng([n_sq, K, ["sparse", "dense", "dup"].index(density)])
    for trial in range(6 if K <= 1024 else 1):
        # groups: runs of templates (in "dup" libraries many templates share a group), numbered by first member
        if density == "dup":
            group_of = np.zeros(K, np.int32)
            firsts = [0]
            for t in range(1, K):
                if rng.random() < 0.5:
                    group_of[t] = group_of[int(rng.integers(0, t))]
                else:
                    group_of[t] = len(firsts)
                    firsts.append(t)
        else:
            group_of = np.arange(K, dtype=np.int32)
        n_groups = int(group_of.max()) + 1
        order = np.argsort(group_of, kind="stable")
        members = order.astype(np.int32)
        group_off = np.searchsorted(group_of[order], np.arange(n_groups + 1)).astype(np.int32)
        per = {"sparse": 2, "dense": 24, "dup": 6}[density]
        n_match = np.zeros(n_sq, np.int32)
        stride = per * 2
        match = np.zeros((n_sq, stride), np.int32)
        hot = rng.integers(0, n_groups, 8)   # squares often repeat a few groups (and group 0)
        for i in range(n_sq):
            if rng.random() < 0.15:
                n_match[i] = -1   # no quad in the crop
                continue
            k = int(rng.integers(0, per + 1))
            gs = set(rng.integers(0, n_groups, k).tolist())
            if rng.random() < 0.5:
                gs |= set(rng.choice(hot, 2).tolist())
            if trial & 1 and i > 0 and rng.random() < 0.3:
                gs.add(0)
            gs = sorted(gs)[:stride]
            n_match[i] = len(gs)
            match[i, :len(gs)] = [g << 2 | int(rng.integers(0, 4)) for g in gs]
        if trial == 0:
            n_match[0] = 0   # first square without a match: the score-0 survivor case
        ok, out = agrees(lib, n_match, match, stride, K, n_groups, group_of, group_off, members)
        assert ok, (n_sq, K, density, trial, out.tolist())
