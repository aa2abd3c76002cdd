"""The GICP kernels of csrc/gicp.hip alone, at their edges: neighbour lists through lio_gicp_neighbours, covariances, pairs, Mahalanobis
matrices through lio_gicp_mahalanobis, and the cost sums -- every point of every case of tests/gicp_edge_cases.py, judged in the device's own
(pool) order, each case run twice on fresh objects.

  lists        the first k places == the k smallest keys (d2 in f32, pool index), places k .. 31 are -1 or later keys: exact, every point
  covariance   finite; |trace(v0 v0^T) - 1| <= 1e-12; eigen-residual and Rayleigh excess (lambda_min by mpmath) <= 8 E, E = what the f64
               route of oracle/gicp.py (numpy eigh and svd) attains against the same long-double covariance, measured per cloud in the run and
               printed; where lambda_1 - lambda_0 > 1e-6 |C| also v0 v0^T (from the matrix, over its trace) within 8 E / gap + 4 * 2^-53 of the
               long-double one per entry (Davis-Kahan; the 4 * 2^-53: the three f64 roundings of forming 1 - g n n, over g).  The 8: cyclic Jacobi on the device and LAPACK on the host are two backward-stable routes a few ulp apart
               behind the same f64 centring; fixed before the device was run, not tuned on its output.
  pairs        == the smallest key over the target, taken iff d2 < f32(max_corr_dist^2): exact, every source point
  Mahalanobis  |device - long-double inverse of (C_B + R C_A R^T)| <= 64 * 1e3 * 2^-53 * |M^-1|_2 per entry (condition at most 1e3: derived)
  H, b, err    long-double sums over the device's own pairs and matrices; per component (64 + 12) 2^-53 sum |addend|, an addend = what one
               source point contributes to the component, formed in long double with the actual e = b - T a; n_corr exact
In the overflow case the one source point at 3e38 (a covariance of size 1e76) is held to "finite" and the trace only, and E of that cloud is
measured without it: every other point of the cloud gets the bounds above.

E per case in input order (tests/test_gicp_edges_cpu.py prints it; target / source):
  k_edges       k3 1.2e-16 / 1.5e-16   k15 2.2e-15 / 3.6e-15   k16 9.8e-16 / 3.2e-15   k17 1.9e-15 / 5.7e-15   k31 1.9e-15 / 1.9e-15
                k32 2.8e-15 / 2.4e-15  (the same cloud at the three grid resolutions)
  n_edges       k20 n20 6.9e-16 / 6.4e-16   n21 3.2e-15 / 1.0e-15   k32 n32 4.6e-16 / 6.4e-16   n33 6.8e-16 / 8.0e-16
  lattice       g1.0 k7 5.7e-16 / 4.8e-16   k20 1.6e-15 / 4.1e-15   g0.3 k7 1.7e-17 / 1.3e-16   k20 1.4e-16 / 3.7e-16
  duplicates    4.6e-16 / 4.5e-15      near_beats_home 8.8e-16 / 1.7e-15     sparse lone 2.2e-16 / 1.0e-16   beyond 2.5e-14 / 1.7e-16
  threshold     exact 4.2e-13 / 1.4e-13   below 1.1e-13 / 1.4e-13   tie 1.2e-15 / 1.4e-13     no_pairs 3.2e-15 / 1.0e-15
  cost_sizes    target 1.5e-15; source 127 3.2e-15  128 1.0e-15  129 9.9e-16  4097 5.0e-16          far_source 2.2e-16 / 2.5e-15
"""
import ctypes as C

import numpy as np
import pytest

import gicp_edge_cases as GC

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in GC.all_cases()}


@pytest.fixture(scope="module")
def lio():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    assert capi.lib().lio_abi_version() >= 17  # lio_gicp_neighbours / lio_gicp_mahalanobis
    return lio


def _same_points(dev, pts):
    key = lambda a: np.sort(np.ascontiguousarray(a[:, :3], np.float32).view([("x", "u4"), ("y", "u4"), ("z", "u4")]).ravel())
    return np.array_equal(key(dev), key(pts))


def _cloud_checks(g, which, pts, k, name, huge=False):
    P, cov = g.download(which)
    assert _same_points(P, pts), name
    nbr = g.neighbours(which)
    P2, cov2 = g.download(which)
    assert np.array_equal(P.view(np.uint32), P2.view(np.uint32)) and np.array_equal(cov.view(np.uint64), cov2.view(np.uint64)), name  # a diagnostic changes nothing
    bad, want = GC.check_lists(P, k, nbr)
    assert bad == 0, (name, which, "points with a wrong neighbour list", bad, len(P))
    skip = np.nonzero(np.abs(P[:, :3]).max(1) > 1e38)[0] if huge else ()
    assert len(skip) == (1 if huge else 0)
    E = GC.oracle_E(P, want, skip=skip)
    fig = GC.check_planes(P, k, cov, E, skip=skip)
    fig["E"] = E
    return P, cov, fig


def run_case(lio, c, overflow_row=None):
    """one run on a fresh object; returns the figures (worst ratio to each bound)"""
    name, k, T, maxd = c["name"], c["k"], c["T"], c["maxd"]
    g = lio.Gicp(grid_resolution=c["res"], max_points=max(len(c["target"]), len(c["source"])), k=k)
    try:
        g.set_target(c["target"])
        g.set_source(c["source"])
        tp, tcov, ft = _cloud_checks(g, 0, c["target"], k, name)
        sp, scov, fs = _cloud_checks(g, 1, c["source"], k, name, huge=overflow_row is not None)
        fig = dict(E_target=ft["E"], E_source=fs["E"], trace=max(ft["trace"], fs["trace"]), cov=max(ft["c_ratio"], fs["c_ratio"]), dk=max(ft["dk_ratio"], fs["dk_ratio"]),
                   determined=ft["determined"] + fs["determined"], points=ft["n"] + fs["n"])
        r = g.linearize(T, max_corr_dist=maxd)
        corr = g.correspondences()
        want, _ = GC.expected_pairs(sp, tp, T, maxd)
        assert np.array_equal(corr, want), (name, "source points with a wrong pair", int((corr != want).sum()))
        if overflow_row is not None:
            assert corr[np.nonzero((sp[:, 0] > 1e38))[0][0]] == -1
        assert r["n_corr"] == int((want >= 0).sum())
        fig["pairs"] = r["n_corr"]
        maha = g.mahalanobis()
        has, inv, nrm = GC.maha_exact(tcov, scov, corr, T)
        fig["maha"] = 0.0
        if len(has):
            ratio = np.abs(maha[has].astype(GC.LD) - inv).max((1, 2)).astype(np.float64) / (64 * 1e3 * GC.EPS * nrm)
            fig["maha"] = float(ratio.max())
            assert fig["maha"] <= 1.0, (name, "mahalanobis", fig["maha"])
        fig["cost"] = _cost_checks(r, GC.cost_exact(sp, tp, corr, maha, T, True), name)
        if "T2" in c:  # the cached path: the same pairs and matrices at a second pose, no derivatives
            r2 = g.linearize(c["T2"], max_corr_dist=maxd, update_corr=False, with_derivatives=False)
            assert np.array_equal(g.correspondences(), corr) and np.array_equal(g.mahalanobis()[has], maha[has])
            ex2 = GC.cost_exact(sp, tp, corr, maha, c["T2"], False)
            assert r2["n_corr"] == ex2["n"]
            fig["cost"] = max(fig["cost"], _ratio(r2["err"], ex2["err"], ex2["err_abs"]))
            assert fig["cost"] <= 1.0, (name, "cached err", fig["cost"])
        if maxd == 0.0:  # 8: no pairs at all
            assert (corr == -1).all() and r["n_corr"] == 0 and not r["H"].any() and not r["b"].any() and r["err"] == 0.0
            guess = np.ascontiguousarray(T, np.float64)
            out, conv, _ = g.align(guess, max_corr_dist=0.0)
            assert np.array_equal(out.view(np.uint64), guess.view(np.uint64)) and conv is False
    finally:
        g.close()
    return fig


def _ratio(dev, exact, abs_sum):
    dev, exact, abs_sum = np.asarray(dev, GC.LD), np.asarray(exact, GC.LD), np.asarray(abs_sum, GC.LD)
    err = np.abs(dev - exact)
    lim = GC.COST_ULPS * GC.LD(GC.EPS) * abs_sum
    if not np.all(err[lim == 0] == 0):
        return np.inf
    return float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0), initial=0.0))


def _cost_checks(r, ex, name):
    assert r["n_corr"] == ex["n"]
    assert np.all(np.isfinite(r["H"])) and np.all(np.isfinite(r["b"])) and np.isfinite(r["err"])
    if ex["n"] == 0:
        assert not r["H"].any() and not r["b"].any() and r["err"] == 0.0
        return 0.0
    worst = max(_ratio(r["H"], ex["H"], ex["H_abs"]), _ratio(r["b"], ex["b"], ex["b_abs"]), _ratio(r["err"], ex["err"], ex["err_abs"]))
    assert worst <= 1.0, (name, "H / b / err", worst)
    return worst


def _report(name, figs):
    for i, f in enumerate(figs):
        print(f"{name} run {i}: E {f['E_target']:.2e} / {f['E_source']:.2e}  ratios to the bounds: covariance {f['cov']:.3f}  Davis-Kahan {f['dk']:.3f} "
              f"({f['determined']} of {f['points']} points determined)  trace {f['trace']:.1e}  mahalanobis {f['maha']:.3f}  H b err {f['cost']:.3f}  pairs {f['pairs']}")


@pytest.mark.parametrize("name", list(CASES))
def test_case(lio, name):
    """every assertion of the module docstring on one case, twice on fresh objects (the pool order may differ between the runs; each run is held
    to its own expectation)"""
    figs = [run_case(lio, CASES[name]) for _ in range(2)]
    _report(name, figs)


def test_overflowing_source_point(lio):
    """a finite source point whose transformed position overflows f32 under a finite pose, no correspondence distance: no pair for that row, the
    exact pair for every other, and the call returns (the corr kernel leaves such a group at entry, and its searches have fixed trip counts)"""
    c = GC.overflow_source()
    _report(c["name"], [run_case(lio, c, overflow_row=c["row"])])


def test_create_refuses_k_outside_3_to_32(lio):
    from lsd_amd import capi

    L = capi.lib()
    for k in (2, 33):
        assert not L.lio_gicp_create(0, C.c_float(1.0), 64, k)
    for k in (3, 32):
        h = L.lio_gicp_create(0, C.c_float(1.0), 64, k)
        assert h
        L.lio_gicp_destroy(h)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def test_refusals_leave_the_object_as_it_was(lio):
    """n = k - 1, a coordinate that is not finite, a pose that is not finite, a max_corr_dist that is negative or NaN: LIO_E_INVALID, and the
    clouds, covariances, pairs and matrices are the ones from before, bit for bit; neighbours before any cloud: LIO_E_STATE"""
    from lsd_amd import capi

    L = capi.lib()
    c = CASES["n_edges/k20/n21"]
    g = lio.Gicp(grid_resolution=1.0, max_points=64, k=20)
    idx = np.zeros((64, 32), np.int32)
    assert L.lio_gicp_neighbours(g.h, 0, _ptr(idx, C.c_int32), 64) == capi.LIO_E_STATE
    g.set_target(c["target"])
    assert L.lio_gicp_neighbours(g.h, 1, _ptr(idx, C.c_int32), 64) == capi.LIO_E_STATE
    g.set_source(c["source"])
    assert L.lio_gicp_neighbours(g.h, 0, _ptr(idx, C.c_int32), 20) == capi.LIO_E_CAPACITY
    r0 = g.linearize(c["T"], max_corr_dist=2.0)

    def state():
        return [a.tobytes() for w in (0, 1) for a in g.download(w)] + [g.correspondences().tobytes(), g.mahalanobis().tobytes(), g.neighbours(0).tobytes()]

    before = state()
    short = np.ascontiguousarray(c["target"][:19])
    assert L.lio_gicp_set_target(g.h, _ptr(short, C.c_float), 19) == capi.LIO_E_INVALID
    assert L.lio_gicp_set_source(g.h, _ptr(short, C.c_float), 19) == capi.LIO_E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = c["target"].copy()
            p[20, axis] = bad
            assert L.lio_gicp_set_target(g.h, _ptr(p, C.c_float), len(p)) == capi.LIO_E_INVALID
            assert L.lio_gicp_set_source(g.h, _ptr(p, C.c_float), len(p)) == capi.LIO_E_INVALID
    p = c["target"].copy()
    p[:, 3] = np.nan  # the intensity is not a coordinate
    H, b, err, nc, out, it, conv = np.zeros(36), np.zeros(6), C.c_double(0), C.c_uint32(0), np.zeros(16), C.c_int(0), C.c_int(0)
    for T, maxd in [(c["T"], -1.0), (c["T"], np.nan), (c["T"], -np.inf)] + [(_with(c["T"], e, v), 2.0) for e in (0, 3, 7, 11) for v in (np.nan, np.inf)]:
        T = np.ascontiguousarray(T, np.float64)
        assert L.lio_gicp_linearize(g.h, _ptr(T, C.c_double), maxd, 1, 1, _ptr(H, C.c_double), _ptr(b, C.c_double), C.byref(err), C.byref(nc)) == capi.LIO_E_INVALID
        assert L.lio_gicp_align(g.h, _ptr(T, C.c_double), None, maxd, _ptr(out, C.c_double), C.byref(it), C.byref(conv)) == capi.LIO_E_INVALID
    assert state() == before
    # ... and it goes on working
    g.set_target(p)
    r1 = g.linearize(c["T"], max_corr_dist=2.0)
    assert r1["n_corr"] == r0["n_corr"] and abs(r1["err"] - r0["err"]) <= 1e-12 * abs(r0["err"]) and state()[0] != before[0]
    g.close()


def _with(T, entry, value):
    T = np.array(T, np.float64).copy()
    T.reshape(-1)[entry] = value
    return T
