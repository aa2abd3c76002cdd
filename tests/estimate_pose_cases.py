"""The rules of the operator's pose hint (get_estimate_pose; include/lio_hip.h, "the operator's pose hint on the device") restated in numpy,
operation by operation: the nearest key frames with their tie rule, the gather, the chunked z sum, the hint matrix and the result logic.
The tests compare the C ABI and the compiled module against these."""
import numpy as np

ESTIMATE_K = 5
D2_MAX = np.float32(400.0)  # 20 m, squared: a key frame is taken up to and including this
SCORE_POSE, SCORE_OK = 5.0, 0.5


def nearest(positions, xy, k=ESTIMATE_K):
    """positions (F, >= 2) f32 key-frame positions, xy the query in f64 -> (ids, d2): the min(k, F) smallest (d2, id), rising.
    d2 in f32: dx = pos_x - (float)x, dy likewise, d2 = dx*dx + dy*dy (z = 0 on both sides); equal distances go to the smaller id."""
    p = np.asarray(positions, np.float32).reshape(len(positions), -1)
    sx, sy = np.float32(xy[0]), np.float32(xy[1])
    dx, dy = (p[:, 0] - sx).astype(np.float32), (p[:, 1] - sy).astype(np.float32)
    d2 = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
    order = np.lexsort((np.arange(len(p)), d2))[: min(int(k), len(p))]
    return order.astype(np.int32), d2[order]


def within_range(ids, d2):
    """step 1 of the estimate: the nearest frames in order, up to the first with d2 > 400"""
    out = []
    for i, d in zip(ids, d2):
        if d > D2_MAX:
            break
        out.append(int(i))
    return out


def gather(clouds, ids):
    """the named clouds back to back, in the order given"""
    parts = [np.asarray(clouds[i], np.float32).reshape(-1, 4) for i in ids]
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


def chunk_sums(z):
    """chunks of 256 consecutive values; lane j holds (double)z[256 c + j], 0 past the end; x[j] += x[j + s] for s = 128, 64, ..., 1"""
    z = np.asarray(z, np.float32).astype(np.float64)
    n_chunks = (len(z) + 255) // 256
    x = np.zeros((n_chunks, 256))
    x.reshape(-1)[: len(z)] = z
    s = 128
    while s > 0:
        x[:, :s] = x[:, :s] + x[:, s:2 * s]
        s >>= 1
    return x[:, 0].copy()


def z_sum(z):
    """the chunk sums added in rising chunk order by one thread"""
    s = np.float64(0.0)
    for c in chunk_sums(z):
        s = s + c
    return s


def z_mean(cloud):
    c = np.asarray(cloud, np.float32).reshape(-1, 4)
    return z_sum(c[:, 2]) / np.float64(len(c))


def hint_matrix(x0, y0, x1, y1):
    """translation (x0, y0, 0), rotation Rz(atan2(y1 - y0, x1 - x0)); None for an arrow of zero length"""
    dx, dy = float(x1) - float(x0), float(y1) - float(y0)
    if not dx * dx + dy * dy > 0.0:
        return None
    a = np.arctan2(dy, dx)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    T[0, 3], T[1, 3] = x0, y0
    return T


def guess_matrix(hint, z_target, z_source):
    """steps 3 and 4: hint z = z_mean(target) - z_mean(source), then the whole matrix rounded to f32"""
    T = np.array(hint, np.float64).reshape(4, 4).copy()
    T[2, 3] = z_target - z_source
    return T, T.astype(np.float32).astype(np.float64)


def result_logic(converged, score):
    """(result, pose_replaced): steps 6 and 7"""
    if not converged:
        return 0, False
    return (1 if score < SCORE_OK else 0), bool(score < SCORE_POSE)


def final_pose(T):
    """getFinalTransformation().cast<double>(): the rigid part through f32, the last row (0, 0, 0, 1)"""
    out = np.array(T, np.float64).reshape(4, 4).astype(np.float32).astype(np.float64)
    out[3] = [0, 0, 0, 1]
    return out


def nearest_cases():
    """(name, positions (F, 3) f32, query xy, k, ids worked by hand, frames within 20 m worked by hand)"""
    ulp_dy = np.float32(0.005524)  # dy*dy = 3.0515e-5: more than half an ulp of 400 (3.0518e-5), so 400 + dy*dy rounds to the next f32
    return [
        # fewer frames than k: all of them, nearest first
        ("three_frames_k5", np.array([[3, 0, 1.8], [1, 0, 1.8], [-2, 0, 1.8]], np.float32), (0.0, 0.0), 5, [1, 2, 0], [1, 2, 0]),
        # frames 1, 2 and 3 at the same f32 distance, frame 0 further: the smaller ids first
        ("equal_distance", np.array([[5, 0, 0], [0, 2, 7.0], [0, -2, -3.0], [2, 0, 0]], np.float32), (0.0, 0.0), 3, [1, 2, 3], [1, 2, 3]),
        # d2 = 400 exactly is taken, one ulp above is not; z does not count (frame 2 is 1 m away in x, y and 90 m above)
        ("edge_of_20_m", np.array([[20, ulp_dy, 0], [20, 0, 0], [1, 0, 90.0], [-30, 0, 0]], np.float32), (0.0, 0.0), 5, [2, 1, 0, 3], [2, 1]),
        # the query is rounded to f32 before the subtraction: 1e-9 beside a frame is on it
        ("query_in_f32", np.array([[1, 1, 0], [1, 1.0000001, 0]], np.float32), (1.0 + 1e-9, 1.0), 2, [0, 1], [0, 1]),
    ]
