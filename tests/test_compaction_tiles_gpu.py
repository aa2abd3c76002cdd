"""The shared stable stream compaction (csrc/device_prims.h) at the sizes where its tile arithmetic can go wrong, through the public API:
one item, the ends of a wave (63, 64, 65), the ends of a tile of 2048 (2047, 2048, 2049) and a fourth tile of one item (3 * 2048 + 1).

The band append is held bit for bit, in input order, to the numpy restatement of test_dense_map_gpu.py; the index build's finite-row filter to
numpy's count and to a k = 1 self-query over distinct points (every finite row finds its own index at distance 0)."""
import numpy as np
import pytest

from test_dense_map_gpu import _need_gpu, _pose, _same, _xform_restated

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1)


@pytest.mark.parametrize("n", SIZES)
def test_band_append_keeps_input_order_at_tile_edges(n):
    _need_gpu()
    from lsd_amd import lio

    rng = np.random.default_rng(100 + n)
    T, _ = _pose(rng, 37.0, [12.5, -3.25, 0.7])
    p = np.concatenate([rng.normal(0, 20, (n, 3)) * [1, 1, 0.2], rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    z = _xform_restated(p, T)[:, 2].astype(np.float64)
    half, none, every = (float(np.median(z)), 1e6), (1e6, 2e6), (-1e6, 1e6)
    want = [_xform_restated(p, T, 255.0, b) for b in (half, none, every)]
    assert len(want[0]) == (n + 1) // 2 and len(want[1]) == 0 and len(want[2]) == n
    c = lio.Cloud()
    sizes = []
    for b in (half, none, every):  # one after the other into the same cloud: each lands behind what is there
        c.append_host(p, T, 255.0, b)
        sizes.append(len(c.download()))
    got = c.download()
    c.close()
    assert sizes == [len(want[0]), len(want[0]), len(want[0]) + n]
    assert _same(got, np.concatenate(want))


@pytest.mark.parametrize("n", SIZES)
def test_index_build_filters_non_finite_rows_at_tile_edges(n):
    _need_gpu()
    from lsd_amd import lio

    rng = np.random.default_rng(200 + n)
    P = rng.normal(0, 10, (n, 3)).astype(np.float32)
    assert len(np.unique(P, axis=0)) == n  # distinct points: no tie decides
    bad = np.nonzero(np.arange(n) % 3 == 1)[0]  # about a third of the rows, one coordinate each
    P[bad, bad % 3] = np.where(bad % 2 == 0, np.nan, np.inf).astype(np.float32)
    fin = np.isfinite(P).all(1)
    x = lio.KnnIndex()
    nf = x.build(P)
    assert nf == int(fin.sum())
    gi, gd = x.query(P[fin], 1)
    x.close()
    assert np.array_equal(np.asarray(gi).reshape(-1), np.nonzero(fin)[0])
    assert (np.asarray(gd).reshape(-1) == 0).all()
