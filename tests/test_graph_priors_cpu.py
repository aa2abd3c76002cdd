"""The pose graph's priors, the parts that need no device: tests/graph_prior_cases.py's analytic Jacobians against its own central
differences, DCS2, the host-only prior error against the restatement, the ABI revision and symbols, the restatement's outlier stage on the GNSS
scene, and the wrapper's new entry points."""
import ctypes as C
import os
import re

import numpy as np

import graph_cases as GC
import graph_prior_cases as PC
from lsd_amd import capi, lio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR_SYMBOLS = ["lio_graph_add_prior", "lio_graph_set_kernel", "lio_graph_priors", "lio_graph_prior_error", "lio_graph_remove_gnss_outliers"]


def _cases(kind, n=200, seed=51):
    """n (t, q, m, plane) of a type, m and plane as the graph keeps them; the node's quaternion takes both signs"""
    rng = np.random.default_rng(seed + kind)
    out = []
    for k in range(n):
        X = GC.random_pose(rng, 2.0, angle=rng.uniform(0, 3.0))
        p = PC.random_prior(rng, 0, X, kind, err=0.3)
        t, q = GC.T_to_tq(X)
        if k % 2:
            q = -q
        out.append((t, q) + PC.normalise_prior(kind, p[3], p[7]))
    return out


def test_prior_jacobians_against_central_differences():
    h = 1e-6
    for kind in (PC.XYZ, PC.QUAT, PC.PLANE):
        worst, n_neg = 0.0, 0
        for (t, q, m, plane) in _cases(kind):
            J = PC.prior_jacobian(kind, t, q, m, plane)
            num = np.zeros((3, 6))
            for c in range(6):
                d = np.zeros(6)
                d[c] = h
                ep = PC.prior_error(kind, *GC.apply_delta(t, q, d), m, plane)
                em = PC.prior_error(kind, *GC.apply_delta(t, q, -d), m, plane)
                num[:, c] = (ep - em) / (2 * h)
            worst = max(worst, np.abs(J - num).max())
            n_neg += (m @ q < 0) if kind == PC.QUAT else (q[3] < 0)
        print("type", kind, "worst |analytic - central difference|", worst)
        assert worst <= 1e-7, (kind, worst)
        assert n_neg >= 50  # both signs of the quaternion were seen


def test_plane_jacobian_rows_are_zero_on_the_pole():
    # u = A^T n_l = (0, 0, 1): r^2 = 0, azimuth undefined: THE PROJECT'S RULE leaves rows 0 and 1 zero
    t, q = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
    J = PC.prior_jacobian(PC.PLANE, t, q, np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.5]))
    assert not J[:2].any() and np.array_equal(J[2], [0, 0, -1, 0, 0, 0])


def test_dcs2_branches():
    assert PC.robustify(3.0, PC.DCS2, 3.0) == (3.0, 1.0)    # s = 1
    assert PC.robustify(0.5, PC.DCS2, 2.0) == (0.5, 1.0)    # s > 1
    rho, rho1 = PC.robustify(6.0, PC.DCS2, 2.0)             # s = 0.5
    assert rho == 1.5 and rho1 == 4 * 4 * (2.0 - 6.0) / 512.0 and rho1 < 0
    # rho' is the derivative of rho where s < 1
    f = lambda c: PC.robustify(c, PC.DCS2, 2.0)[0]
    assert abs((f(6.0 + 1e-6) - f(6.0 - 1e-6)) / 2e-6 - rho1) < 1e-9
    assert PC.robustify(9.0, PC.HUBER, 1.0) == GC.robustify(9.0, GC.HUBER, 1.0) and PC.dcs_scale(6.0, 2.0) == 0.5


def test_prior_error_agrees_with_the_restatement():
    rng = np.random.default_rng(52)
    worst = 0.0
    for kind in (PC.XYZ, PC.QUAT, PC.PLANE):
        n_flip = 0
        for k in range(100):
            X = GC.random_pose(rng, 2.0)
            p = PC.random_prior(rng, 0, X, kind, err=0.3)
            m = -p[3] if (kind == PC.QUAT and k % 2) else p[3]   # raw, not normalised; both signs of the measured quaternion
            got = lio.PoseGraph.prior_error(X, kind, m, p[7])
            t, q = GC.T_to_tq(X)
            mm, pl = PC.normalise_prior(kind, m, p[7])
            worst = max(worst, np.abs(got - PC.prior_error(kind, t, q, mm, pl)).max())
            n_flip += kind == PC.QUAT and mm @ q < 0
        assert kind != PC.QUAT or n_flip >= 5
    print("worst difference", worst)
    assert worst <= 1e-13
    X = np.eye(4)
    L, p64 = capi.lib(), lambda a: capi.ptr(a, C.c_double)
    e, z4 = np.zeros(3), np.zeros(4)
    assert L.lio_graph_prior_error(p64(X), PC.QUAT, p64(z4), None, p64(e)) == capi.LIO_E_INVALID
    assert L.lio_graph_prior_error(p64(X), PC.PLANE, p64(np.array([0.0, 0, 1, 0])), None, p64(e)) == capi.LIO_E_INVALID
    assert L.lio_graph_prior_error(p64(X), 3, p64(z4), None, p64(e)) == capi.LIO_E_INVALID


def test_abi_revision_and_prior_symbols():
    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    assert int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1)) >= 15 and capi.lib().lio_abi_version() >= 15
    for name in PRIOR_SYMBOLS:
        assert hasattr(capi.lib(), name) and name in hdr and name in capi.SYMBOLS, name
    for name, value in (("KERNEL_DCS2", 2), ("PRIOR_XYZ", 0), ("PRIOR_QUAT", 1), ("PRIOR_PLANE", 2)):
        assert int(re.search(r"#define LIO_GRAPH_%s (\d+)" % name, hdr).group(1)) == value == getattr(capi, "GRAPH_" + name)
    assert (lio.PoseGraph.DCS2, lio.PoseGraph.XYZ, lio.PoseGraph.QUAT, lio.PoseGraph.PLANE) == (PC.DCS2, PC.XYZ, PC.QUAT, PC.PLANE)
    for name in ("add_prior", "set_kernel", "priors", "prior_error", "remove_gnss_outliers"):
        assert callable(getattr(lio.PoseGraph, name))


def test_restatement_outlier_stage_on_the_gnss_scene():
    spec = PC.spec_gnss()
    g = PC.build(spec, PC.Graph())
    assert PC.Graph().remove_gnss_outliers() == (None, {}, {})
    removed, rep, scales = g.remove_gnss_outliers(1.0, 100, min_edges=1)
    print("planted", spec["planted"], "scales", scales)
    assert removed == spec["planted"] and len(removed) == 2
    assert all(s < 0.1 for k, s in scales.items() if k in removed) and all(s > 1.5 for k, s in scales.items() if k not in removed)
    assert [p["id"] for p in g.priors()] == [k for k in scales if k not in removed] and all(p["kernel"] == PC.DCS2 and p["delta"] == 20.0 for p in g.priors())
    worst = max(GC.pose_diff(a, b)[0] for a, b in zip(g.estimates(), spec["truth"]))
    assert worst < 0.5


def test_wrapper_prior_entries_with_the_switch_off():
    import slam_wrapper as sw

    assert hasattr(sw, "add_graph_gnss") and hasattr(sw, "_graph_priors")
    assert sw._graph_priors() == [] and sw.run_robust_graph_optimization("mapping") == {}
    assert sw.add_graph_gnss(0, np.zeros(3), 1.0, 3) == []
