"""Ground extraction (csrc/ground.hip, lio_ground_*; slam_wrapper.set_ground_extraction / _detect_ground), the parts that need no GPU: the
ABI revision and symbols, the refusals without a device, the default of accumulate_cloud(extract_ground=True), and the draw generator
against known answers."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ground_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lio_hip.h")

GROUND_SYMBOLS = ["lio_ground_default_params", "lio_ground_draw", "lio_ground_create", "lio_ground_destroy", "lio_ground_detect_scan",
                  "lio_ground_detect_host", "lio_ground_download_indices", "lio_ground_download_normals", "lio_ground_download_inliers",
                  "lio_ground_download_draws", "lio_ground_last_run", "lio_ground_last_times"]

# (seed, draw, points) -> the three indices by include/lio_hip.h's rule, recorded when the rule was written (a change of the generator shows here)
KNOWN_DRAWS = [
    ((0, 0, 3), (2, 1, 0)),
    ((0, 1, 1000), (202, 173, 352)),
    ((7, 63, 49351), (43054, 11527, 15256)),
    ((123456789, 1000, 1024), (335, 574, 141)),
    ((0xFFFFFFFF, 10999, 2 ** 31 - 1), (1489584196, 479416363, 159219997)),
]


def _module():
    import slam_wrapper

    assert slam_wrapper.__file__.endswith(".so")
    return slam_wrapper


@pytest.fixture
def ground_switch():
    sw = _module()
    yield sw
    sw.set_ground_extraction(False)


def test_header_and_library_are_at_revision_9_with_every_ground_symbol():
    from lsd_amd import capi

    hdr = int(re.search(r"#define LIO_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert hdr >= 9 and capi.lib().lio_abi_version() == hdr
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lio_ground_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(GROUND_SYMBOLS)
    for n in GROUND_SYMBOLS:
        assert n in capi.SYMBOLS and hasattr(capi.lib(), n)


def test_params_layout_and_presets_match_the_header():
    from lsd_amd import capi, lio

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lio_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(lio_ground_params), ' \
          'offsetof(lio_ground_params, k), offsetof(lio_ground_params, seed)); return 0; }'
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, off_k, off_seed = (int(x) for x in subprocess.check_output([exe]).decode().split())
    assert size == C.sizeof(capi.GroundParams) and off_k == capi.GroundParams.k.offset and off_seed == capi.GroundParams.seed.offset
    p0, p1 = lio.GroundDetector.params(0), lio.GroundDetector.params(1, seed=5)
    assert (p0.clip_low, p0.clip_high, p1.clip_low, p1.clip_high) == (1.5, 1.5, 2.0, 1.0)  # graph_utils.cpp:331-332, floor_detection_nodelet.cpp:40-41
    for p in (p0, p1):
        assert (p.sensor_height, p.use_normal_filter, p.normal_thresh_deg, p.k, p.distance_threshold, p.min_points, p.floor_normal_thresh_deg,
                p.max_iterations, p.probability) == (0.0, 1, 20.0, 10, 0.1, 1024, 10.0, 1000, 0.99)
    assert p0.seed == 0 and p1.seed == 5
    with pytest.raises(ValueError):
        lio.GroundDetector.params(0, no_such_field=1)


def test_detector_without_a_device_raises():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() > 0:
        pytest.skip("a HIP device is visible: covered by tests/test_ground_gpu.py")
    with pytest.raises(capi.LioError):
        lio.GroundDetector()


def test_draws_against_known_answers():
    """three restatements of the rule (the library's host function, numpy in lio.ground_draw, Python integers in the test helper) and the
    committed answers; the indices are distinct and in range"""
    from lsd_amd import capi, lio

    out = (C.c_uint32 * 3)()
    for (seed, j, n), want in KNOWN_DRAWS:
        capi.lib().lio_ground_draw(seed, j, n, out)
        assert tuple(out) == want and gc.draw(seed, j, n) == want and tuple(lio.ground_draw(seed, j, n)) == want
    js = np.arange(5000)
    for seed, n in ((0, 3), (1, 4), (99, 1024), (2 ** 32 - 1, 66117)):
        t = lio.ground_draw(seed, js, n)
        assert t.min() >= 0 and t.max() < n
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
        for j in (0, 1, 4999):
            capi.lib().lio_ground_draw(seed, j, n, out)
            assert tuple(out) == tuple(t[j]) == gc.draw(seed, j, n)
    h = np.bincount(lio.ground_draw(3, np.arange(200_000), 1000).reshape(-1), minlength=1000)  # every index is drawn, roughly uniformly
    assert h.min() > 400 and h.max() < 800


def test_module_surface_and_the_default_refusal(ground_switch):
    sw = ground_switch
    assert callable(sw.set_ground_extraction) and callable(sw._detect_ground)
    assert "PCL" in sw.set_ground_extraction.__doc__
    pts = np.zeros((10, 4), np.float32)
    pa = {"points_attr": np.zeros((10, 2), np.float32), "timestamp": 0}
    rows = np.array([[0, 0, 0, 0, 0, 0, 0, 1.0], [1000, 0, 0, 0, 0, 0, 0, 1.0]])
    with pytest.raises(ValueError, match="extract_ground.*set_ground_extraction"):
        sw.accumulate_cloud(pts, pa, rows, "TUM", True)
    sw.set_ground_extraction(True, 3)
    sw.set_ground_extraction(False)
    with pytest.raises(ValueError, match="extract_ground"):
        sw.accumulate_cloud(pts, pa, rows, "TUM", True)


def test_switch_on_without_a_device_is_a_clear_error(ground_switch, tmp_path):
    from lsd_amd import capi

    if capi.lib().lio_device_count() > 0:
        pytest.skip("a HIP device is visible: covered by tests/test_ground_gpu.py")
    sw = ground_switch
    pts = np.zeros((10, 4), np.float32)
    pa = {"points_attr": np.zeros((10, 2), np.float32), "timestamp": 0}
    rows = np.array([[0, 0, 0, 0, 0, 0, 0, 1.0], [1000, 0, 0, 0, 0, 0, 0, 1.0]])
    sw.set_ground_extraction(True, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        sw.accumulate_cloud(pts, pa, rows, "TUM", True)
    with pytest.raises(RuntimeError, match="HIP device"):
        sw._detect_ground(pts)
    f = tmp_path / "nothing.pcd"
    sw.save_accumulate_cloud(str(f), 0.0)  # nothing was accumulated
    assert not f.exists()


def test_restated_plane_and_loop_on_a_small_cloud():
    """the helper itself: a bad draw for duplicated and collinear points, a plane through three points, the loop's early stop"""
    assert gc.plane([0, 0, 0], [1, 1, 1], [2, 2, 2]) is None and gc.plane([1, 2, 3], [1, 2, 3], [4, 5, 6]) is None
    assert gc.plane([0, 0, 0], [np.inf, 0, 0], [0, 1, 0]) is None
    pl = gc.plane([0, 0, 1], [1, 0, 1], [0, 1, 1])
    assert np.array_equal(pl, np.array([0, 0, 1, -1], np.float32))
    rng = np.random.default_rng(0)
    P = np.column_stack([rng.uniform(-10, 10, (2000, 2)), rng.normal(0, 0.01, 2000)]).astype(np.float32)
    tri, counts, planes, run = gc.ransac(P, 5, 64)
    assert run["winner"] >= 0 and run["skipped"] == 0 and 1 <= run["iterations"] <= 10 and counts[run["winner"]] > 1900
    assert np.array_equal(gc.residual_ok(P, planes[run["winner"]]).sum(), counts[run["winner"]])
