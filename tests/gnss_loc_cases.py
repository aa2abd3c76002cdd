"""GNSS in localisation mode, restated in numpy / plain Python from the reference's statements, independent of the library:

  update_origin   graph_update_origin's coordinate change (hdl_graph_slam_nodelet.cpp:1396-1449) over rtk_cases.UtmRef
  InsList         the localiser's ins_data: ins_callback (hdl_localization_nodelet.cpp:81-87) and the bracket rule of :231-261
  nearest_ten     the kd-tree query of GlobalLocalization::localSearch under the project's rule (include/lio_hip.h, lio_sc_local_search)
  local_walk      the sequential walk of global_localization.cpp:366-381
  local_search    the whole of localSearch over sc_cases

and the seeded cases the tests share.  Scalars are Python floats (IEEE f64, one rounding per operation, left to right like the C++)."""
import numpy as np

import rtk_cases as rc
import sc_cases as sc

# (from, to) origins as (latitude, longitude, altitude): 1e-5 degrees apart, (3e-4, 4e-4, 2 m), (5e-3, -7e-3, -12.5 m)
ORIGIN_A = (31.2304, 121.4737, 14.0)
ORIGIN_PAIRS = tuple((ORIGIN_A, (ORIGIN_A[0] + dlat, ORIGIN_A[1] + dlon, ORIGIN_A[2] + dalt))
                     for dlat, dlon, dalt in ((1e-5, 1e-5, 0.0), (3e-4, 4e-4, 2.0), (5e-3, -7e-3, -12.5)))


def update_origin(origin_from, origin_to, poses=None, xyz=None):
    """a map under origin_from expressed under origin_to: (poses (n, 4, 4), xyz (m, 3)) as f64 copies; rotations untouched"""
    pf, pt = rc.UtmRef(), rc.UtmRef()
    zf = pf.forward(origin_from[0], origin_from[1])
    zt = pt.forward(origin_to[0], origin_to[1])

    def move(x, y, z):
        lat, lon = pf.inverse(x + zf[0], y + zf[1])
        nx, ny = pt.forward(lat, lon)
        return nx - zt[0], ny - zt[1], z + origin_from[2] - origin_to[2]

    P = np.array(poses if poses is not None else np.zeros((0, 4, 4)), np.float64).reshape(-1, 4, 4)
    X = np.array(xyz if xyz is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3)
    for k in range(len(X)):
        X[k] = move(float(X[k, 0]), float(X[k, 1]), float(X[k, 2]))
    for k in range(len(P)):
        P[k, :3, 3] = move(float(P[k, 0, 3]), float(P[k, 1, 3]), float(P[k, 2, 3]))
    return P, X


def seeded_poses(seed=11, n=200, half=400.0):
    """n poses within +-half metres of an origin, any rotation"""
    rng = np.random.default_rng(seed)
    P = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        P[k, :3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        P[k, :3, 3] = [rng.uniform(-half, half), rng.uniform(-half, half), rng.uniform(-5.0, 5.0)]
    return P


def seeded_map(origin_a, origin_b, seed=11, n=200, half=400.0):
    """(poses under origin_a, the same poses under origin_b): n places within about +-half metres of origin_a given by latitude / longitude, each
    projected FORWARD under either origin with a projector pinned by that origin -- no inverse projection enters, so either set is exact to the
    projector's forward rounding; the heights differ by the origins' altitudes"""
    rng = np.random.default_rng(seed)
    PA = seeded_poses(seed, n, half)
    PB = PA.copy()
    pa, pb = rc.UtmRef(), rc.UtmRef()
    za, zb = pa.forward(origin_a[0], origin_a[1]), pb.forward(origin_b[0], origin_b[1])
    for k in range(n):
        lat = origin_a[0] + float(rng.uniform(-half, half)) / 111000.0
        lon = origin_a[1] + float(rng.uniform(-half, half)) / 95000.0
        xa, ya = pa.forward(lat, lon)
        xb, yb = pb.forward(lat, lon)
        PA[k, 0, 3], PA[k, 1, 3] = xa - za[0], ya - za[1]
        PB[k, 0, 3], PB[k, 1, 3] = xb - zb[0], yb - zb[1]
        PB[k, 2, 3] = PA[k, 2, 3] + origin_a[2] - origin_b[2]
    return PA, PB


class InsList:
    """ins_data of the localiser: entries are dicts with stamp_us, T (4 x 4), precision, dimension"""

    def __init__(self):
        self.data = []

    def push(self, entry):  # ins_callback
        if len(self.data) >= 10:
            del self.data[0]
        self.data.append(entry)

    def stamps(self):
        return [e["stamp_us"] for e in self.data]

    def observe(self, stamp):
        """the bracket rule for a scan's stamp (us): None, or dict(T, precision, dimension, ratio, first, second); clears the list when the stamp is
        beyond its last entry"""
        d = self.data
        if not d:
            return None
        if stamp > d[-1]["stamp_us"]:
            d.clear()
            return None
        if not stamp >= d[0]["stamp_us"]:
            return None
        first, second, valid = 0, 0, False
        while second != len(d):
            dt = (float(d[first]["stamp_us"]) - float(stamp)) / 1000000.0
            dt2 = (float(d[second]["stamp_us"]) - float(stamp)) / 1000000.0
            if dt <= 0 and dt2 >= 0 and (dt2 - dt) < 0.2:
                valid = True
                break
            first = second
            second += 1
        if not valid:
            return None
        a, b = d[first], d[second]
        ratio = float(stamp - a["stamp_us"]) / float(b["stamp_us"] - a["stamp_us"] + 1)
        return dict(T=rc.interpolate_transform(a["T"], b["T"], ratio), precision=a["precision"], dimension=a["dimension"], ratio=ratio,
                    first=a["stamp_us"], second=b["stamp_us"])


def position_d2(pos, ins_xy):
    """f32 squared distance of every frame (F, 3) to (f32(x), f32(y), 0): ((dx*dx) + dy*dy) + dz*dz"""
    p = np.asarray(pos, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - np.float32(ins_xy[0]), p[:, 1] - np.float32(ins_xy[1]), p[:, 2]
        return ((dx * dx) + dy * dy) + dz * dz


def nearest_ten(pos, ins_xy):
    """(ids, d2) of the min(10, F) nearest frames in rising (d2, id); what is not a number sorts after every number"""
    d2 = position_d2(pos, ins_xy)
    key = (d2.view(np.uint32).astype(np.uint64) & np.uint64(0x7FFFFFFF)) << np.uint64(32) | np.arange(len(d2), dtype=np.uint64)
    order = np.argsort(key, kind="stable")[:sc.CANDIDATES]
    return order.astype(np.int64), d2[order]


def local_walk(ids, d2, dist, shifts, precision):
    """global_localization.cpp:366-381 -> (match id or -1, shift, score, n_examined)"""
    best, best_shift, min_dist, examined = -1, 0, 1.0, 0
    p2 = float(precision) * float(precision)
    for i in range(len(ids)):
        if best == -1 and float(d2[i]) > p2:
            return -1, 0, min_dist, examined
        if best != -1 and float(d2[i]) > p2 / 10.0:
            break
        examined += 1
        if dist[i] < min_dist:
            min_dist, best, best_shift = float(dist[i]), int(ids[i]), int(shifts[i])
    return best, best_shift, min_dist, examined


def local_search(cloud, bank_clouds, pos, ins_xy, precision):
    """localSearch -> dict(match_id, shift, yaw, score, n_examined, ids, d2, dist, shifts); only the nearest frames' clouds are described"""
    ids, d2 = nearest_ten(pos, ins_xy)
    if len(ids) == 0:
        return dict(match_id=-1, shift=0, yaw=sc.shift_to_yaw(0), score=1.0, n_examined=0, ids=ids, d2=d2, dist=np.zeros(0), shifts=np.zeros(0, np.int64))
    desc = sc.describe(cloud)
    dist, shifts, _ = sc.distance(np.repeat(desc[None], len(ids), 0), np.stack([sc.describe(bank_clouds[i]) for i in ids]))
    m, s, score, n = local_walk(ids, d2, dist, shifts, precision)
    return dict(match_id=m, shift=s, yaw=sc.shift_to_yaw(s), score=score, n_examined=n, ids=ids, d2=d2, dist=dist, shifts=shifts)


# ---- the bank of the device test --------------------------------------------------------------------------------------------------------------
def local_bank(n):
    """(clouds, positions): n frames of 150 points each, on a 3 m grid of positions (50 to a row) with modest heights"""
    rng = np.random.default_rng(100 + n)
    c = np.concatenate([rng.uniform(-60, 60, (n, 150, 2)), rng.uniform(0.0, 6.0, (n, 150, 1)), np.zeros((n, 150, 1))], 2).astype(np.float32)
    clouds = [np.ascontiguousarray(x) for x in c]
    k = np.arange(n)
    pos = np.stack([3.0 * (k % 50) + rng.uniform(-0.5, 0.5, n), 3.0 * (k // 50) + rng.uniform(-0.5, 0.5, n), rng.uniform(-0.3, 0.3, n)], 1).astype(np.float32)
    return clouds, pos


def query_of(cloud, seed, n_new=30, yaw_deg=None):
    """a scan that looks like `cloud`: the same points but for n_new fresh ones, turned about z by yaw_deg (seeded when None)"""
    rng = np.random.default_rng(seed)
    q = np.array(cloud, np.float64)
    q[:n_new] = np.concatenate([rng.uniform(-60, 60, (n_new, 2)), rng.uniform(0.0, 6.0, (n_new, 1)), np.zeros((n_new, 1))], 1)
    a = np.radians(float(rng.choice([0.0, 43.0, 180.0, 291.0])) if yaw_deg is None else yaw_deg)
    x, y = q[:, 0].copy(), q[:, 1].copy()
    q[:, 0], q[:, 1] = np.cos(a) * x - np.sin(a) * y, np.sin(a) * x + np.cos(a) * y
    return q.astype(np.float32)
