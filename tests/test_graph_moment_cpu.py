"""The GNSS moment stage of the pose graph, the parts that need no device: tests/graph_moment_cases.py's analytic Jacobians against central
differences, the sign convention, the restatement's recovery of a planted lever arm on the seeded scenes, the ABI revision and symbols, the
wrapper's switch, and the calls' loud failure without a device."""
import os
import re

import numpy as np
import pytest

import graph_cases as GC
import graph_moment_cases as MC
from lsd_amd import capi, lio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENT_SYMBOLS = ["lio_graph_estimate_gnss_moment", "lio_graph_moment_begin", "lio_graph_moment_end", "lio_graph_moment_get", "lio_graph_moment_linearize"]


def test_moment_jacobians_against_central_differences():
    rng = np.random.default_rng(71)
    h, worst = 1e-6, 0.0
    for k in range(200):
        t, q = GC.T_to_tq(GC.random_pose(rng, 3.0, angle=rng.uniform(0, 3.0)))
        if k % 2:
            q = -q
        z, m = rng.normal(0, 3.0, 3), rng.normal(0, 1.0, 3)
        J, Jm = MC.moment_jacobians(t, q, z, m)
        num, num_m = np.zeros((3, 6)), np.zeros((3, 3))
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            num[:, c] = (MC.moment_error(*GC.apply_delta(t, q, d), z, m) - MC.moment_error(*GC.apply_delta(t, q, -d), z, m)) / (2 * h)
        for c in range(3):
            d = np.zeros(3)
            d[c] = h
            num_m[:, c] = (MC.moment_error(t, q, z, m + d) - MC.moment_error(t, q, z, m - d)) / (2 * h)
        worst = max(worst, np.abs(J - num).max(), np.abs(Jm - num_m).max())
    print("worst |analytic - central difference|", worst)
    assert worst <= 1e-7


def test_sign_convention_fixes_at_t_plus_R_l_give_minus_l():
    """noise-free: three fixed poses with different orientations and fixes z = t + R l; the stage's optimum is m = -l up to the pull of the
    moment's loose prior at 0, and the moved measurements are the poses' own positions"""
    rng = np.random.default_rng(72)
    lever = np.array([0.6, -0.3, 0.4])
    g = MC.Graph()
    X = [GC.random_pose(rng, 5.0) for _ in range(3)]
    for T in X:
        n = g.add_node(T, fixed=True)
        g.add_prior(n, MC.XYZ, T[:3, 3] + T[:3, :3] @ lever, np.eye(3) / 0.05)
    n, m, rep = g.estimate_gnss_moment(min_edges=1)
    print("moment", m, "report", rep)
    assert n == 3 and np.abs(m + lever).max() < 1e-3 and np.abs(m - lever).max() > 0.5
    for p, T in zip(g.priors(), X):
        assert p["kernel"] == MC.DCS2 and p["delta"] == 20.0 and np.abs(p["measurement"][:3] - T[:3, 3]).max() < 1e-3
    assert g.moment is None


@pytest.mark.parametrize("name", list(MC.SCENES))
def test_restatement_recovers_the_lever_arm(name):
    """the condition on the committed scenes: |m + l| < 0.15 m in the restatement alone, after the outlier stage took the two displaced fixes"""
    spec = MC.spec_moment(**MC.SCENES[name])
    ref = MC.reference(name)
    miss = np.linalg.norm(ref["moment"] + spec["lever"])
    worst = max(np.linalg.norm(a[:3, 3] - b[:3, 3]) for a, b in zip(ref["estimates"], spec["truth"]))
    print(name, "moment", ref["moment"], "|m + l|", miss, "report", {k: v for k, v in ref["report"].items() if k != "history"}, "largest position error", worst)
    assert ref["removed"] == spec["planted"] and len(ref["removed"]) == 2 and ref["priors"] == 18
    assert miss < 0.15
    assert worst < 0.5
    assert ref["report"]["trials"] > ref["report"]["accepted"]  # a rejected trial: the restore of m is exercised


def test_restatement_edge_conditions():
    g = MC.build(MC.spec_moment(n=12, outliers=()), MC.Graph())
    before = [p["measurement"].copy() for p in g.priors()]
    g.moment_begin([0.1, 0.2, 0.3])
    assert g.n_live() == len([e for e in g.edges if e["live"]]) + 1
    g.optimize(2, min_edges=1)
    assert g.moment_end(apply=False) == 0 and all(np.array_equal(a, p["measurement"]) for a, p in zip(before, g.priors()))
    empty = MC.Graph()
    empty.add_node(np.eye(4))
    assert empty.estimate_gnss_moment()[0] == 0
    assert g.estimate_gnss_moment(min_edges=100)[0] is None


def test_abi_revision_and_moment_symbols():
    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    assert int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1)) >= 25 and capi.lib().lio_abi_version() >= 25
    for name in MOMENT_SYMBOLS:
        assert hasattr(capi.lib(), name) and name in hdr and name in capi.SYMBOLS, name
    for name in ("estimate_gnss_moment", "moment_begin", "moment_end", "moment", "linearize_moment"):
        assert callable(getattr(lio.PoseGraph, name))
    assert "m = -l" in hdr  # the sign convention is stated where the rules are


def test_wrapper_switch_exists_and_is_inert_without_a_graph():
    import slam_wrapper as sw

    assert hasattr(sw, "set_gnss_moment") and hasattr(sw, "_last_gnss_moment")
    assert sw._last_gnss_moment() == {}
    assert sw.run_robust_graph_optimization("mapping") == {} and sw._last_gnss_moment() == {}


def test_every_call_fails_loudly_without_a_device():
    if capi.lib().lio_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(capi.LioError):
        lio.PoseGraph()
    L = capi.lib()
    m = np.zeros(3)
    assert L.lio_graph_estimate_gnss_moment(None, 1.0, 10, None, capi.ptr(m, capi.C.c_double), None) == capi.LIO_E_INVALID
    assert L.lio_graph_moment_begin(None, None, None) == capi.LIO_E_INVALID
    assert L.lio_graph_moment_end(None, 1) == capi.LIO_E_INVALID
    assert L.lio_graph_moment_get(None, capi.ptr(m, capi.C.c_double)) == capi.LIO_E_INVALID
    assert L.lio_graph_moment_linearize(None, None, None, None, 0) == capi.LIO_E_INVALID
