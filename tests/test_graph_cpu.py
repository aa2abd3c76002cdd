"""The pose graph, the parts that need no device: the ABI revision and symbols, the host helpers (fromVectorMQT, toVectorMQT, the edge error)
against tests/graph_cases.py's f64 restatement, the restatement's analytic Jacobians against its own central differences, and the wrapper's
graph entry points with the switch off."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graph_cases as GC
from lsd_amd import capi, lio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAPH_SYMBOLS = ["lio_graph_default_params", "lio_graph_create", "lio_graph_destroy", "lio_graph_reset", "lio_graph_add_node", "lio_graph_set_fixed",
                 "lio_graph_set_estimate", "lio_graph_add_edge", "lio_graph_remove_edge", "lio_graph_optimize", "lio_graph_estimates", "lio_graph_edges",
                 "lio_graph_chi2", "lio_graph_linearize", "lio_graph_last_times", "lio_se3_from_mqt", "lio_se3_to_mqt", "lio_graph_edge_error",
                 "lio_loop_pair_information"]


def _poses():
    """200 seeded poses; among them the identity, rotations within 1e-3 .. 1e-9 of pi, and rotations whose matrix -> quaternion conversion
    comes out with w < 0 before the sign is chosen"""
    rng = np.random.default_rng(11)
    out = [np.eye(4)]
    for eps in (1e-3, 1e-6, 1e-9, 0.0):
        for _ in range(6):
            out.append(GC.random_pose(rng, 1.0, angle=np.pi - eps))
    while len(out) < 200:
        out.append(GC.random_pose(rng, 1.0))
    return out


POSES = _poses()


def test_abi_revision_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 13 and capi.lib().lio_abi_version() == rev
    for name in GRAPH_SYMBOLS:
        assert hasattr(capi.lib(), name) and name in hdr and name in capi.SYMBOLS, name
    assert C.sizeof(capi.GraphParams) == 24 and C.sizeof(capi.GraphReport) == 64
    p = lio.PoseGraph.default_params()
    assert (p.min_edges, p.cg_epsilon, p.chi2_rel_stop, p.cg_max_iterations) == (10, 1e-10, 0.0, 0)


def test_to_and_from_mqt_agree_with_the_restatement():
    n_wneg = 0
    for T in POSES:
        v = lio.PoseGraph.to_mqt(T)
        assert np.abs(v - GC.to_mqt(T)).max() <= 1e-14
        assert np.abs(lio.PoseGraph.from_mqt(v) - GC.from_mqt(v)).max() <= 1e-14
        if 1.0 - v[3:] @ v[3:] > 1e-12:  # (at a half turn w^2 = 1 - |q|^2 is rounding noise of either sign: the vector does not carry the angle back)
            assert np.abs(lio.PoseGraph.from_mqt(v) - T).max() <= 1e-7
        # the conversion's own sign: Eigen's branch for a negative trace can give w < 0
        R = T[:3, :3]
        if np.trace(R) <= 0:
            i = int(np.argmax(np.diag(R)))
            j, k = (i + 1) % 3, (i + 2) % 3
            n_wneg += (R[k, j] - R[j, k]) < 0
    assert n_wneg >= 5


def test_edge_error_agrees_with_the_restatement():
    worst, n_flip = 0.0, 0
    for k in range(len(POSES)):
        Xi, Xj, M = POSES[k], POSES[(k * 7 + 3) % len(POSES)], POSES[(k * 13 + 5) % len(POSES)]
        e = lio.PoseGraph.edge_error(Xi, Xj, M)
        want = GC.edge_eval(*GC.T_to_tq(Xi), *GC.T_to_tq(Xj), *GC.T_to_tq(M))[0]
        worst = max(worst, np.abs(e - want).max())
        # the two routes of the restatement (quaternions, 4 x 4 matrices) are the same function; a rotation within 1e-6 of pi is left out: there
        # x, y, z lose half the digits of w and the sign choice is on the edge
        viaT = GC.edge_error_T(Xi, Xj, M)
        if 1.0 - want[3:] @ want[3:] > 1e-6:
            assert np.abs(viaT - want).max() <= 1e-13
        qraw = GC.q_mul(GC.q_conj(GC.T_to_tq(M)[1]), GC.q_mul(GC.q_conj(GC.T_to_tq(Xi)[1]), GC.T_to_tq(Xj)[1]))
        n_flip += qraw[3] < 0
    assert worst <= 1e-14
    assert n_flip >= 20  # the sign choice was exercised
    assert np.abs(lio.PoseGraph.edge_error(POSES[3], POSES[3], np.eye(4))).max() <= 1e-15


def test_analytic_jacobians_against_central_differences():
    h, worst = 1e-6, 0.0
    rng = np.random.default_rng(12)
    for k in range(60):
        (ti, qi), (tj, qj), (mt, mq) = [GC.T_to_tq(GC.random_pose(rng, 1.0, angle=rng.uniform(0, 2.5))) for _ in range(3)]
        if k % 3 == 0:  # the error quaternion's raw w is negative: the sign branch of the Jacobian
            mq = -mq
        Ji, Jj = GC.jacobians(ti, qi, tj, qj, mt, mq)
        num_i, num_j = np.zeros((6, 6)), np.zeros((6, 6))
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            ep = GC.edge_eval(*GC.apply_delta(ti, qi, d), tj, qj, mt, mq)[0]
            em = GC.edge_eval(*GC.apply_delta(ti, qi, -d), tj, qj, mt, mq)[0]
            num_i[:, c] = (ep - em) / (2 * h)
            ep = GC.edge_eval(ti, qi, *GC.apply_delta(tj, qj, d), mt, mq)[0]
            em = GC.edge_eval(ti, qi, *GC.apply_delta(tj, qj, -d), mt, mq)[0]
            num_j[:, c] = (ep - em) / (2 * h)
        worst = max(worst, np.abs(Ji - num_i).max(), np.abs(Jj - num_j).max())
    assert worst <= 1e-7, worst


def test_from_mqt_beyond_the_unit_ball_is_the_identity_rotation():
    v = np.array([0.3, -0.2, 0.1, 0.8, 0.5, 0.4])  # |q| > 1
    T = lio.PoseGraph.from_mqt(v)
    assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], v[:3]) and np.array_equal(T, GC.from_mqt(v))
    t, q = GC.apply_delta(np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), v)
    assert np.array_equal(q, [0, 0, 0, 1]) and np.array_equal(t, v[:3])


def test_restatement_huber_and_lm_on_a_small_graph():
    assert GC.robustify(0.25, GC.HUBER, 1.0) == (0.25, 1.0)
    rho, rho1 = GC.robustify(9.0, GC.HUBER, 1.0)
    assert rho == 5.0 and rho1 == 1.0 / 3.0
    g = GC.build(GC.spec_ring(), GC.Graph())
    assert g.optimize(10, min_edges=13)[0] == -1
    it, rep = g.optimize(50, min_edges=1)
    assert rep["chi2_final"] < 1e-18 < rep["chi2_initial"]
    for X, T in zip(g.estimates(), GC.spec_ring()["truth"]):
        assert GC.pose_diff(X, T)[0] < 1e-9


def test_graph_needs_a_device_or_says_so():
    if capi.lib().lio_device_count() > 0:
        lio.PoseGraph().close()
        return
    with pytest.raises(capi.LioError, match="no CPU fallback"):
        lio.PoseGraph()


def test_wrapper_graph_entries_with_the_switch_off():
    import slam_wrapper as sw

    assert sw.get_graph_edges() == {} and sw.run_graph_optimization() == {}
    assert sw.get_graph_meta() == {} or set(sw.get_graph_meta()) == {"vertex", "edge"}
    assert hasattr(sw, "set_pose_graph")
