"""The operator's pose hint on the device through the C ABI: lio_localmap_nearest / _gather / _z_mean against the numpy restatement
(tests/estimate_pose_cases.py) to the last bit, lio_gicp_set_target_device / _set_source_device against the host entries to the last bit in
everything downstream (the pool order included), and lio_localmap_estimate_pose against the same matcher driven by hand with clouds assembled on the host."""
import ctypes as C

import numpy as np
import pytest

import estimate_pose_cases as E
from lsd_amd import capi, lio, synth

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _cloud(n, seed):
    """n points whose z spans six decades with both signs, so that the order of the z sum shows in its last bits"""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 5.0, (n, 4)).astype(np.float32)
    c[:, 2] = (rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    return c


SIZES = [0, 1, 255, 256, 257, 63, 64, 65, 1000, 0]  # the two sets of the gather: frames 0 .. 4 and 5 .. 9


@pytest.fixture(scope="module")
def store():
    lm = lio.LocalMap(max_total_points=4096, max_local_points=8, max_keyframe_points=1000)  # the gather's buffer: max(1008, 5 * 1000) points
    clouds = [_cloud(n, 100 + k) for k, n in enumerate(SIZES)]
    for k, c in enumerate(clouds):
        assert lm.add_keyframe(c, [float(k), 0.0, 0.0]) == k
    yield lm, clouds
    lm.close()


def _gather_rc(lm, ids):
    i = np.ascontiguousarray(ids, np.int32)
    n, z = C.c_uint32(0), C.c_double(0)
    return capi.lib().lio_localmap_gather(lm.h, capi.ptr(i, C.c_int32), len(i), C.byref(n), C.byref(z))


@pytest.mark.parametrize("ids", [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [4, 0, 2, 1, 3], [8, 9, 5], [1], [3, 3, 4, 3], [6, 2, 6, 8, 0, 1, 4, 7, 5, 9, 3, 1, 1, 0, 9, 2]])
def test_gather_and_z_mean_to_the_last_bit(store, ids):
    lm, clouds = store
    want = E.gather(clouds, ids)
    n, z = lm.gather(ids)
    got = lm.download_gather()
    assert n == len(want) and _same(got, want)
    assert _same(np.float64(z), np.float64(E.z_mean(want))), (z, E.z_mean(want))
    n2, z2 = lm.gather(ids)  # the same call twice: the same bits
    assert n2 == n and _same(np.float64(z2), np.float64(z)) and _same(lm.download_gather(), got)
    p, m = lm.gather_device()
    assert p and m == n and _same(np.float64(lm.z_mean(p, m)), np.float64(z))  # the second entry runs the same sum over a cloud where it lies


def test_gather_limits(store):
    lm, clouds = store
    n, z = lm.gather([2, 7])
    before = lm.download_gather()
    assert _gather_rc(lm, [8] * 6) == capi.LIO_E_CAPACITY  # 6000 points into a buffer of 5000
    assert _same(lm.download_gather(), before) and lm.gather_device()[1] == n
    assert _gather_rc(lm, [0, 9]) == capi.LIO_E_INVALID and _gather_rc(lm, []) == capi.LIO_E_INVALID  # a total of 0
    assert _gather_rc(lm, [0] * 17) == capi.LIO_E_INVALID and _gather_rc(lm, [10]) == capi.LIO_E_INVALID and _gather_rc(lm, [-1]) == capi.LIO_E_INVALID
    assert _same(lm.download_gather(), before)
    assert lm.gather([8] * 5)[0] == 5000  # exactly the buffer


def test_nearest_entry_against_the_hand_worked_cases():
    for name, pos, xy, k, want_ids, want_near in E.nearest_cases():
        lm = lio.LocalMap(max_total_points=64, max_local_points=8, max_keyframe_points=8)
        try:
            for p in pos:
                lm.add_keyframe(np.zeros((0, 4), np.float32), p)
            ids, d2 = lm.nearest(xy, k)
            rids, rd2 = E.nearest(pos, xy, k)
            assert ids.tolist() == want_ids == rids.tolist() and _same(d2, rd2), name
            assert E.within_range(ids, d2) == want_near, name
            assert len(lm.nearest(xy, 0)[0]) == 0
            bad = np.array([np.nan, 0.0])
            assert capi.lib().lio_localmap_nearest(lm.h, capi.ptr(bad, C.c_double), 1, capi.ptr(np.zeros(1, np.int32), C.c_int32), None) == capi.LIO_E_INVALID
        finally:
            lm.close()


# ---- the device setters -------------------------------------------------------------------------------------------------------------------

def _holder(clouds):
    """clouds put on the device: a local map whose kept frames (slots 0 and 1) are two of them"""
    lm = lio.LocalMap(max_total_points=sum(len(c) for c in clouds) + 16, max_local_points=8, max_keyframe_points=max(len(c) for c in clouds))
    for c in clouds:
        lm.add_keyframe(c, [0.0, 0.0, 0.0])
    return lm


def _ptr_of(lm, frame):
    n, _ = lm.gather([frame])
    p, m = lm.gather_device()
    assert p and m == n
    return p, n


@pytest.fixture(scope="module")
def pair():
    scene = synth.Scene(half=6.0, n_boxes=4, seed=11, box_size=(1.0, 3.0), keep_clear=1.0)
    tgt = scene.sample_surface(300, seed=12).astype(np.float32).reshape(-1, 4)
    src = scene.sample_surface(200, seed=13).astype(np.float32).reshape(-1, 4)
    a = 0.03
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    src[:, :3] = ((src[:, :3].astype(np.float64) - [0.1, -0.05, 0.02]) @ R).astype(np.float32)  # the source = the scene seen from a pose a little off
    nan = src.copy()
    nan[77, 1] = np.nan
    lm = _holder([tgt, src, nan, src[:19]])
    yield lm, tgt, src
    lm.close()


def _canon(pts, cov):
    """the cloud of a download in an order of its own: rows sorted by their bits (x, then y, z, intensity)"""
    o = np.lexsort(_bits(pts).T[::-1])
    return pts[o], cov[o]


@pytest.fixture(scope="module", params=[0.0, 1.0], ids=["gicp", "vgicp"])
def setters(pair, request):
    """the same 300-point target and 200-point source set from the host (gh) and from the device (gd), and what both answer from one guess"""
    lm, tgt, src = pair
    gh, gd = lio.Gicp(grid_resolution=1.0, max_points=512, k=20), lio.Gicp(grid_resolution=1.0, max_points=512, k=20)
    for g in (gh, gd):
        if request.param:
            g.set_voxel_mode(request.param, 1)
    gh.set_target(tgt)
    gh.set_source(src)
    p, n = _ptr_of(lm, 0)
    assert n == 300
    gd.set_target_device(p, n)
    p, n = _ptr_of(lm, 1)
    assert n == 200
    gd.set_source_device(p, n)
    guess = np.eye(4)
    guess[:3, 3] = [0.05, 0.0, 0.0]

    def answers(g):
        out = [g.download(0), g.download(1)]
        T, conv, it = g.align(guess, max_corr_dist=1.0)
        return dict(clouds=out, T=T, converged=conv, iterations=it, fitness=g.fitness_score(T, 25.0))

    yield dict(lm=lm, gh=gh, gd=gd, host=answers(gh), device=answers(gd), answers=answers)
    gh.close()
    gd.close()


def test_device_setters_bit_for_bit(setters):
    """lio_gicp_download of both sides (points and covariances), lio_gicp_align's T, converged and iterations from the same guess, and
    lio_gicp_fitness_score with its count: equal bit for bit between the host and the device entry.  This holds because set_target / set_source
    put the grid's pool into the one order the cloud defines (cells by their lowest row, points by row): the grid's own arrival order differs
    from one insertion to the next, and with it differed the downloads (181 to 283 of these 300 rows) and T (1e-15 to 2e-15)."""
    h, d = setters["host"], setters["device"]
    for which in (0, 1):
        assert _same(h["clouds"][which][0], d["clouds"][which][0]) and _same(h["clouds"][which][1], d["clouds"][which][1]), which
    print(f"host: converged {h['converged']} in {h['iterations']} iterations, fitness {h['fitness']}; device: {d['converged']} {d['iterations']} {d['fitness']}")
    assert _same(h["T"], d["T"]) and (h["converged"], h["iterations"]) == (d["converged"], d["iterations"])
    assert _same(np.float64(h["fitness"][0]), np.float64(d["fitness"][0])) and h["fitness"][1] == d["fitness"][1] and h["fitness"][1] > 0


def test_setting_a_cloud_again_repeats_the_pool(pair):
    """the same cloud set three times on one handle and once on another, from either side: one download.  The pool holds every point once"""
    lm, tgt, src = pair
    g1, g2 = lio.Gicp(grid_resolution=1.0, max_points=512, k=20), lio.Gicp(grid_resolution=1.0, max_points=512, k=20)
    try:
        g1.set_target(tgt)
        first = g1.download(0)
        assert _same(_canon(*first)[0], tgt[np.lexsort(_bits(tgt).T[::-1])])
        for _ in range(2):
            g1.set_target(tgt)
            again = g1.download(0)
            assert _same(first[0], again[0]) and _same(first[1], again[1])
        g2.set_source_device(*_ptr_of(lm, 0))
        other = g2.download(1)
        assert _same(first[0], other[0]) and _same(first[1], other[1])
    finally:
        g1.close()
        g2.close()


def test_device_setters_refuse_what_the_host_entries_refuse(setters):
    """a cloud with one NaN, a cloud below k points and one above max_points are refused, and the matcher still answers as before the call"""
    L, lm, gd = capi.lib(), setters["lm"], setters["gd"]
    before = setters["answers"](gd)
    p, n = _ptr_of(lm, 2)
    assert L.lio_gicp_set_source_device(gd.h, C.c_void_p(p), n) == capi.LIO_E_INVALID
    assert L.lio_gicp_set_target_device(gd.h, C.c_void_p(p), n) == capi.LIO_E_INVALID
    p, n = _ptr_of(lm, 3)
    assert n == 19 and L.lio_gicp_set_source_device(gd.h, C.c_void_p(p), n) == capi.LIO_E_INVALID
    assert L.lio_gicp_set_target_device(gd.h, C.c_void_p(p), 513) == capi.LIO_E_CAPACITY
    assert L.lio_gicp_set_target_device(gd.h, None, 300) == capi.LIO_E_INVALID
    after = setters["answers"](gd)
    for which in (0, 1):  # the clouds were not touched: this handle's own pool, row for row
        assert _same(before["clouds"][which][0], after["clouds"][which][0]) and _same(before["clouds"][which][1], after["clouds"][which][1])
    assert _same(before["T"], after["T"]) and (before["converged"], before["iterations"]) == (after["converged"], after["iterations"])
    assert _same(np.float64(before["fitness"][0]), np.float64(after["fitness"][0]))


# ---- lio_localmap_estimate_pose -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def town():
    """six key frames 4 m apart along x, a scan taken between the third and the fourth"""
    scene = synth.Scene(half=30.0, n_boxes=24, seed=7, keep_clear=11.0)  # no box over the key frames
    frames, positions = [], []
    for k in range(6):
        pos = np.array([-10.0 + 4.0 * k, 0.0, 1.8])
        raw, _ = synth.make_scan(scene, pos, synth.quat_from_rotvec([0, 0, 0]), seed=40 + k, n_az=100, fov_deg=(-24.8, 2.0))
        w = raw.copy()
        w[:, :3] = (raw[:, :3].astype(np.float64) + pos).astype(np.float32)
        frames.append(w)
        positions.append(pos.astype(np.float32))
    true_pos, true_yaw = np.array([0.3, 0.2, 1.8]), 0.02
    src, _ = synth.make_scan(scene, true_pos, synth.quat_from_rotvec([0, 0, true_yaw]), seed=60, n_az=100, fov_deg=(-24.8, 2.0))
    lm = lio.LocalMap(max_total_points=sum(len(f) for f in frames) + 16, max_local_points=8, max_keyframe_points=max(len(f) for f in frames))
    for f, p in zip(frames, positions):
        lm.add_keyframe(f, p)
    holder = _holder([src])
    holder.store_frame(0, *_ptr_of(holder, 0))
    lp = capi.LoopParams()
    capi.lib().lio_loop_default_params(C.byref(lp))
    cap = 5 * max(len(f) for f in frames)
    gd, gh = lio.Gicp(lp.grid_resolution, cap, lp.k_correspondences), lio.Gicp(lp.grid_resolution, cap, lp.k_correspondences)
    for g in (gd, gh):
        g.set_voxel_mode(lp.voxel_resolution, 1)
    yield dict(lm=lm, frames=frames, positions=np.array(positions), src=src, holder=holder, gd=gd, gh=gh, lp=lp, true_pos=true_pos, true_yaw=true_yaw)
    for h in (gd, gh, holder, lm):
        h.close()


def _by_hand(t, hint):
    """the parent's matcher with clouds assembled on the host, from the guess the rules give"""
    ids = E.within_range(*E.nearest(t["positions"], (hint[0, 3], hint[1, 3])))
    target = E.gather(t["frames"], ids)
    T0, guess = E.guess_matrix(hint, E.z_mean(target), E.z_mean(t["src"]))
    g, lp = t["gh"], t["lp"]
    g.set_target(target)
    g.set_source(t["src"])
    prm = capi.NdtParams()
    capi.lib().lio_estimate_matcher_params(C.byref(prm))
    T, conv, it = g.align(guess, max_corr_dist=1.0, rotation_epsilon_deg=prm.rotation_epsilon_deg, transformation_epsilon=prm.transformation_epsilon,
                          max_iterations=prm.max_iterations, max_process_time_ms=prm.max_process_time_ms)
    score = g.fitness_score(T, lp.fitness_score_max_range)[0] if conv else 0.0
    result, replaced = E.result_logic(conv, score)
    return dict(ids=ids, n_target=len(target), guess=guess, T=T, converged=conv, iterations=it, score=score, result=result,
                out=E.final_pose(T) if replaced else T0)


def test_estimate_pose_is_the_matcher_driven_by_hand(town):
    t = town
    a = t["true_yaw"] + np.radians(2.0)
    hint = E.hint_matrix(t["true_pos"][0] + 0.2, t["true_pos"][1] - 0.15, t["true_pos"][0] + 0.2 + np.cos(a), t["true_pos"][1] - 0.15 + np.sin(a))
    want = _by_hand(t, hint)
    p, n = t["holder"].frame(0)
    out, r = t["lm"].estimate_pose(t["gd"], p, n, hint)
    print("estimate:", {k: v for k, v in r.items() if k != "guess"}, "\nout_T\n", out)
    assert r["ids"] == want["ids"] and len(r["ids"]) == 5 and r["n_target"] == want["n_target"] and r["n_source"] == len(t["src"])
    assert _same(np.float64(r["z_mean_target"]), np.float64(E.z_mean(E.gather(t["frames"], want["ids"]))))
    assert _same(np.float64(r["z_mean_source"]), np.float64(E.z_mean(t["src"])))
    assert _same(r["guess"], want["guess"])
    assert (bool(r["converged"]), r["iterations"], r["result"]) == (want["converged"], want["iterations"], want["result"])
    assert _same(np.float64(r["score"]), np.float64(want["score"])) and _same(out, want["out"])
    assert r["result"] == E.result_logic(r["converged"], r["score"])[0] and bool(r["pose_replaced"]) == E.result_logic(r["converged"], r["score"])[1]
    # the scene is the map's and the hint is 0.25 m and 2 degrees off: the match is a good one, and it lands on the truth
    assert r["result"] == 1 and np.linalg.norm(out[:3, 3] - t["true_pos"]) < 0.1
    assert all(r[k] >= 0.0 for k in ("nearest_us", "gather_us", "set_target_us", "set_source_us", "z_source_us", "align_us", "fitness_us")) and r["gather_us"] > 0.0
    out2, r2 = t["lm"].estimate_pose(t["gd"], p, n, hint)  # again: the same bits
    assert _same(out2, out) and _same(np.float64(r2["score"]), np.float64(r["score"])) and r2["iterations"] == r["iterations"]


def test_estimate_pose_far_from_every_key_frame(town):
    t = town
    hint = E.hint_matrix(35.5, 0.0, 36.5, 0.5)  # 25.5 m beyond the last key frame
    p, n = t["holder"].frame(0)
    out, r = t["lm"].estimate_pose(t["gd"], p, n, hint)
    assert r["result"] == 0 and r["ids"] == [] and r["n_target"] == 0 and not r["converged"] and _same(out, hint)
    out, r = t["lm"].estimate_pose(t["gd"], None, 0, E.hint_matrix(0.0, 0.0, 1.0, 0.0))  # no source: the same answer, whatever is near
    assert r["result"] == 0 and r["n_target"] == 0 and len(r["ids"]) == 5 and _same(out, E.hint_matrix(0.0, 0.0, 1.0, 0.0))
