"""tools/check_bench_dump.py on dumps written by bench.py's own dump_outputs (CPU): a dump of the oracle's results passes, a dump
with one record or one count changed fails and names the frame."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import helpers as H

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import check_bench_dump as CBD  # noqa: E402
from opencv_ar_amd import MARKER_DTYPE  # noqa: E402


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_dump", os.path.join(H.ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """config 2 (640x480, 2x2 template), 5 distinct frames tiled over a 13-frame batch, 8 records per frame, as bench.py dumps"""
    cfg, names, uniq, n = H.synth_config(2), ["2x2-01"], 5, 13
    tpls, cam = H.oracle_templates(names), H.oracle_camera(cfg.width, cfg.height)
    refs = [H.oracle_registration(H.synth_frame(cfg, i, names)[0], tpls, cam)[0] for i in range(uniq)]
    markers, counts = np.zeros((n, 8), MARKER_DTYPE), np.zeros(n, np.int32)
    for f in range(n):
        ref = refs[f % uniq]
        counts[f] = len(ref)
        for k, r in enumerate(ref[:8]):
            markers[f, k] = np.frombuffer(bytes(r), MARKER_DTYPE)[0]
        markers[f, len(ref):] = markers[f, 0]   # (slots past the count: dump_outputs zeroes them)
    d = str(tmp_path_factory.mktemp("dump"))
    _bench().dump_outputs(d, markers, counts)
    assert counts.sum() >= n
    return d, uniq, counts


def test_oracle_results_pass(dump):
    d, uniq, counts = dump
    assert CBD.check_dump(d, config=2, unique=uniq) == (len(counts), int(counts.sum()))


@pytest.mark.parametrize("field", ["counts", "score", "square", "glMatrix"])
def test_a_changed_output_fails(dump, tmp_path, field):
    d, uniq, counts = dump
    for f in os.listdir(d):
        np.save(os.path.join(tmp_path, f), np.load(os.path.join(d, f)))
    f = int(np.flatnonzero(counts)[-1])   # the last frame with a marker
    a = np.load(os.path.join(tmp_path, field + ".npy"))
    if field == "counts":
        a[f] += 1
    elif field == "glMatrix":
        a[f, 0, 12] += 1e-3 * max(1.0, np.abs(a[f, 0]).max())
    elif field == "square":
        a[f, 0, 3] += 1.0
    else:
        a[f, 0] = np.nextafter(a[f, 0], np.inf)
    np.save(os.path.join(tmp_path, field + ".npy"), a)
    with pytest.raises(AssertionError, match=f"batch frame {f} "):
        CBD.check_dump(str(tmp_path), config=2, unique=uniq)
