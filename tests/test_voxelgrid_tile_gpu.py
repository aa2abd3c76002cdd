"""The downsample chain sums every voxel whose run of points lies inside one staged half (1024 points) of a 2048-point sort tile from LDS, inside
vg_heads_*; only runs that cross an edge of such a half travel through the `sorted` buffer and the long-run / monster queues, and the first radix pass makes the point indices itself (no index
array is written beside the keys).  Here both forms of the chain (one scan, batched) against the oracle, bit for bit, on clouds whose SORTED layout is
built on purpose: a cloud is a list of (cell, count) in ascending voxel-key order, so every run's start and length relative to the tile edges is
known -- and asserted on the CPU before the GPU sees the cloud -- then the rows are permuted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAF = 0.5
TILE = 2048
MAX_N = 12000


def fill(total, size, first_cell=0):
    """runs of `size` points (the last one shorter) holding `total` points, cells first_cell, first_cell + 1, ..."""
    runs, c = [], first_cell
    while total > 0:
        runs.append((c, min(size, total)))
        total -= runs[-1][1]
        c += 1
    return runs


def after(runs, more):
    """`more` (a list of counts, or of (cell, count) with cells counted from 0) behind `runs`, in the cells that follow"""
    c0 = runs[-1][0] + 1 if runs else 0
    out = list(runs)
    for k, m in enumerate(more):
        out.append((c0 + m[0], m[1]) if isinstance(m, tuple) else (c0 + k, m))
    return out


def build(runs, n_bad=0, seed=0, far_row=None):
    """cells lie along x (cell c = [c / 2, c / 2 + 1 / 2) m), so the voxel key is the cell number minus the first; far_row = a row of cells further up
    in y for the last run, which multiplies the cell count of the box (more radix passes) without changing the order"""
    rng = np.random.default_rng(seed)
    parts = []
    for k, (c, m) in enumerate(runs):
        y0 = far_row * LEAF if (far_row is not None and k == len(runs) - 1) else 0.0
        parts.append(np.column_stack([c * LEAF + rng.uniform(0.05, 0.45, m), y0 + rng.uniform(0.05, 0.45, m), rng.uniform(0.05, 0.45, m), rng.uniform(0, 255, m)]))
    cloud = np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 4), np.float32)
    if n_bad:
        bad = np.column_stack([rng.uniform(0, 10, n_bad), rng.uniform(0, 1, n_bad), rng.uniform(0, 1, n_bad), rng.uniform(0, 255, n_bad)]).astype(np.float32)
        bad[np.arange(n_bad), rng.integers(0, 3, n_bad)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), n_bad)
        cloud = np.concatenate([cloud, bad])
    assert 0 < len(cloud) <= MAX_N
    return np.ascontiguousarray(cloud[rng.permutation(len(cloud))])


def sorted_layout(cloud):
    """(start, length) of every run in sorted position and the radix passes the box needs, from the definition of the voxel key (f32 as the chain)"""
    ok = np.isfinite(cloud[:, :3]).all(1)
    p = cloud[ok, :3]
    if len(p) == 0:
        return [], 0
    inv = np.float32(1.0 / LEAF)
    minb = np.floor(p.min(0) * inv).astype(np.int64)
    div = np.floor(p.max(0) * inv).astype(np.int64) - minb + 1
    ijk = np.floor(p * inv).astype(np.int64) - minb
    key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    ks = np.sort(key, kind="stable")
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    lens = np.diff(np.r_[starts, len(ks)])
    total = int(div.prod())
    return list(zip(starts.tolist(), lens.tolist())), (total.bit_length() + 7) // 8


def check_layout(cloud, runs, want_runs_at=()):
    """the construction holds on the CPU: the runs are the intended ones, and the named (start, length) pairs are among them"""
    layout, passes = sorted_layout(cloud)
    assert [m for _, m in layout] == [m for _, m in runs]
    for sl in want_runs_at:
        assert sl in layout, (sl, layout[:8])
    return layout, passes


_pool = []


@pytest.fixture(scope="module", autouse=True)
def _free_the_pool():
    yield
    while _pool:
        _pool.pop().close()


def scans(k):
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device")
    while len(_pool) < k:
        _pool.append(lio.Scan(max_raw=16384, max_ds=16384))
    return _pool[:k]


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def check_single(oracle_mod, s, cloud):
    want = oracle_mod.voxel_downsample(cloud, LEAF)
    s.upload(cloud)
    n = s.voxel_downsample(LEAF)
    assert n == len(want)
    got = s.get_ds()
    assert same(got, want), np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[:5]
    return want


def check_batch(oracle_mod, clouds):
    from lsd_amd import lio

    ss = scans(len(clouds))
    for s, c in zip(ss, clouds):
        s.upload(c)
    ns = lio.Scan.voxel_downsample_batch(ss, LEAF)
    for k, (s, c, n) in enumerate(zip(ss, clouds, ns)):
        want = oracle_mod.voxel_downsample(c, LEAF)
        assert n == len(want), k
        got = s.get_ds()
        assert same(got, want), (k, np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[:5])


FIVE = [(0, 2), (1, 1), (2, 2)]  # a 5-point scan


def both_forms(oracle_mod, cloud):
    check_single(oracle_mod, scans(1)[0], cloud)
    check_batch(oracle_mod, [cloud, build(FIVE, seed=5)])


# ---- 1. runs at the tile edge --------------------------------------------------------------------------------------------------------------------
def test_run_ends_at_2047_and_the_next_starts_at_2048(oracle_mod):
    runs = after(fill(TILE, 8), [5, 3, 40, 1])
    cloud = build(runs, seed=11)
    check_layout(cloud, runs, [(2040, 8), (2048, 5)])
    both_forms(oracle_mod, cloud)


def test_two_point_run_starts_at_2047(oracle_mod):
    runs = after(fill(2047, 23), [2, 7, 35])
    cloud = build(runs, seed=12)
    check_layout(cloud, runs, [(2047, 2), (2049, 7)])
    both_forms(oracle_mod, cloud)


@pytest.mark.parametrize("m", [31, 32, 33])
def test_run_of_about_a_wave_starts_at_2040(oracle_mod, m):
    runs = after(fill(2040, 8), [m, 4, 4])
    cloud = build(runs, seed=13 + m)
    check_layout(cloud, runs, [(2040, m)])
    both_forms(oracle_mod, cloud)


# ---- 1b. the same at the edges of the staged half tiles: vg_heads stages 1024 points at a time, a run across the middle of a tile crosses too ----------
HALF_EDGES = [TILE // 2, TILE + TILE // 2]


@pytest.mark.parametrize("edge", HALF_EDGES)
def test_run_ends_just_before_a_half_tile_edge_and_the_next_starts_on_it(oracle_mod, edge):
    runs = after(fill(edge, 8), [5, 3, 40, 1])
    cloud = build(runs, seed=111 + edge)
    check_layout(cloud, runs, [(edge - 8, 8), (edge, 5)])
    both_forms(oracle_mod, cloud)


@pytest.mark.parametrize("edge", HALF_EDGES)
def test_two_point_run_starts_just_before_a_half_tile_edge(oracle_mod, edge):
    runs = after(fill(edge - 1, 23), [2, 7, 35])
    cloud = build(runs, seed=112 + edge)
    check_layout(cloud, runs, [(edge - 1, 2), (edge + 1, 7)])
    both_forms(oracle_mod, cloud)


@pytest.mark.parametrize("edge", HALF_EDGES)
@pytest.mark.parametrize("m", [31, 32, 33])
def test_run_of_about_a_wave_starts_eight_before_a_half_tile_edge(oracle_mod, m, edge):
    runs = after(fill(edge - 8, 8), [m, 4, 4])
    cloud = build(runs, seed=113 + m + edge)
    check_layout(cloud, runs, [(edge - 8, m)])
    both_forms(oracle_mod, cloud)


@pytest.mark.parametrize("edge", HALF_EDGES)
@pytest.mark.parametrize("last", [3, 40])
def test_last_valid_run_ends_on_a_half_tile_edge_before_non_finite_rows(oracle_mod, last, edge):
    runs = after(fill(edge - last, 6), [last])
    cloud = build(runs, n_bad=700, seed=114 + last + edge)
    layout, _ = check_layout(cloud, runs, [(edge - last, last)])
    assert sum(m for _, m in layout) == edge
    both_forms(oracle_mod, cloud)


# ---- 2. run lengths around the two thresholds, at a tile start and mid-tile -------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, TILE, 1000])
@pytest.mark.parametrize("m", [31, 32, 33, 2047, 2048, 2049])
def test_run_lengths_around_the_thresholds(oracle_mod, m, start):
    runs = after(fill(start, 8), [m, 3, 33, 6])
    cloud = build(runs, seed=m + start)
    check_layout(cloud, runs, [(start, m)])
    both_forms(oracle_mod, cloud)


def test_a_middle_tile_without_a_head(oracle_mod):
    runs = after(fill(1000, 5), [5000, 9, 40, 2])
    cloud = build(runs, seed=21)
    layout, _ = check_layout(cloud, runs, [(1000, 5000)])
    assert not any(TILE <= a < 2 * TILE for a, _ in layout)  # tile 1 holds points 2048 .. 4095 of the long run only
    both_forms(oracle_mod, cloud)


# ---- 3. the run table's capacity, the smallest clouds -------------------------------------------------------------------------------------------------
def test_2048_one_point_voxels_in_one_tile(oracle_mod):
    for runs in (fill(TILE, 1), after(fill(TILE, 1), [7, 1, 1])):
        cloud = build(runs, seed=31)
        layout, _ = check_layout(cloud, runs)
        assert layout[:TILE] == [(k, 1) for k in range(TILE)]
        both_forms(oracle_mod, cloud)


@pytest.mark.parametrize("n", [1, 5, 2048, 2049, 4097])
def test_smallest_clouds_and_one_voxel_clouds(oracle_mod, n):
    for runs in (fill(n, 3), fill(n, n)):
        cloud = build(runs, seed=32 + n)
        assert len(cloud) == n
        check_layout(cloud, runs)
        both_forms(oracle_mod, cloud)


# ---- 4. non-finite rows ----------------------------------------------------------------------------------------------------------------------------
def nonfinite_clouds():
    mid = after(fill(2990, 7), [10])                      # the last valid run ends at 3000: mid-tile
    edge = after(fill(2 * TILE - 40, 6), [40])            # ... at 4096: exactly a tile edge (a long run that must not be taken to go on)
    edge_short = after(fill(2 * TILE - 3, 9), [3])
    return [(mid, 300), (edge, 300), (edge_short, 2500), (None, 2500)]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_non_finite_rows(oracle_mod, which):
    runs, n_bad = nonfinite_clouds()[which]
    if runs is None:  # no finite row at all: no radix pass, no voxel
        cloud = build([], n_bad=n_bad, seed=44)
        assert sorted_layout(cloud) == ([], 0)
        assert len(oracle_mod.voxel_downsample(cloud, LEAF)) == 0
    else:
        cloud = build(runs, n_bad=n_bad, seed=40 + which)
        layout, _ = check_layout(cloud, runs)
        assert sum(m for _, m in layout) == (3000 if which == 0 else 2 * TILE)
    both_forms(oracle_mod, cloud)


# ---- 5. one Scan, reused: stale `sorted` and index contents ------------------------------------------------------------------------------------------
def test_the_same_scan_large_then_small_then_nothing(oracle_mod):
    from lsd_amd import lio

    s = lio.Scan(max_raw=16384, max_ds=16384)
    big = build(after(fill(3000, 11), [5000, 2049, 30, 30, 1800]), seed=51)
    small = build(FIVE, seed=52)
    nothing = build([], n_bad=700, seed=53)
    for cloud in (big, small, nothing, small, big, nothing):
        check_single(oracle_mod, s, cloud)
    other = lio.Scan(max_raw=16384, max_ds=16384)
    for a, b in ((big, small), (small, nothing), (nothing, big), (small, big)):
        s.upload(a)
        other.upload(b)
        ns = lio.Scan.voxel_downsample_batch([s, other], LEAF)
        for sc, c, n in zip((s, other), (a, b), ns):
            want = oracle_mod.voxel_downsample(c, LEAF)
            assert n == len(want) and same(sc.get_ds(), want)


# ---- 6. batched: whole and partial groups of eight scans ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 8, 9])
def test_batched_groups_of_eight(oracle_mod, k):
    nf = nonfinite_clouds()
    menu = [build(after(fill(TILE, 8), [5, 3, 40, 1]), seed=61),
            build(FIVE, seed=62),
            build(after(fill(2040, 8), [33, 4, 4]), seed=63),
            build(after(fill(1000, 5), [5000, 9, 40, 2]), seed=64),
            build([], n_bad=900, seed=65),
            build(after(fill(TILE, 1), [7, 1, 1]), seed=66),
            build(nf[1][0], n_bad=nf[1][1], seed=67),
            build(fill(4097, 4097), seed=68),
            build(after(fill(2047, 23), [2, 2049, 31]), seed=69)]
    check_batch(oracle_mod, [menu[(j + k) % len(menu)] for j in range(k)])


# ---- 7. a sort launched with fewer radix passes than the box needs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,then", [(1, 2), (1, 3), (2, 3)])
def test_under_launched_sort_is_run_again(oracle_mod, first, then):
    """A scan's chain launches as many radix passes as its previous cloud needed (lio_scan_voxel_downsample; the batch takes the largest of its
    scans' counts).  A narrow cloud first, then one whose box needs more: the first try leaves the keys unsorted and -- the indices being born in pass
    0 -- the index buffer it would read partly unwritten or stale; it must touch neither, report "again", and the re-run must equal the oracle."""
    from lsd_amd import lio

    shapes = {1: (fill(900, 5), None),                                            # 180 cells: 8 bits
              2: (after(fill(3000, 4), [(3000, 2100), (3001, 37)]), None),        # 3752 cells: 12 bits
              3: (after(fill(3000, 4), [(500, 2100), (501, 37)]), 60)}            # 1252 x 61 cells: 17 bits
    clouds = {}
    for need, (runs, far) in shapes.items():
        clouds[need] = build(runs, seed=70 + need, far_row=far)
        _, passes = check_layout(clouds[need], runs)
        assert passes == need
    a, b = lio.Scan(max_raw=16384, max_ds=16384), lio.Scan(max_raw=16384, max_ds=16384)
    for s in (a, b):
        check_single(oracle_mod, s, clouds[first])  # the scan now predicts `first` passes
    check_single(oracle_mod, a, clouds[then])
    check_single(oracle_mod, a, clouds[first])
    b.upload(clouds[then])
    a.upload(clouds[first])
    ns = lio.Scan.voxel_downsample_batch([a, b], LEAF)  # a predicts `first` again, b still does: the batch launches `first`
    for s, c, n in zip((a, b), (clouds[first], clouds[then]), ns):
        want = oracle_mod.voxel_downsample(c, LEAF)
        assert n == len(want) and same(s.get_ds(), want)
