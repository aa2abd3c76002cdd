"""The rules of the colour map (include/lio_hip.h, "Colour map on the device"; MapRender of slam/localization/map_render) restated in numpy,
operation by operation, plus the seeded cases the tests run.  Every f64 sum of products is written out left to right (numpy and Python
floats round every operation on its own, as the library built without contraction does), so the device has to agree bit for bit.

The ground test is not restated here (tests/ground_cases.py does that for the detector): `Painter.frame` takes the floor inliers from a
callable, and the device tests hand it the device detector with the painter's parameters."""
import functools
import math

import numpy as np

POINT_RES = 0.02
INV_POINT_RES = 1.0 / POINT_RES
VOXEL_RES = 0.2
INV_VOXEL_RES = 1.0 / VOXEL_RES
MIN_DEPTH, MAX_DEPTH = 2.0, 80.0
MARGIN = 0.005
BOX_LIMIT = 1 << 20
MIN_MOVE = 0.1
GROUND_THRESHOLD = 0.2  # detect_ground's RANSAC threshold in map_render.cpp (graph_utils.cpp uses 0.1)


# ---- small exact pieces ------------------------------------------------------------------------------------------------------------------
def round_half_away(x):
    """std::round on f64: the fraction is exact, so no double rounding"""
    x = np.asarray(x, np.float64)
    t = np.trunc(x)
    with np.errstate(invalid="ignore"):
        return t + np.sign(x) * (np.abs(x - t) >= 0.5)


def mulv(a, v):
    return np.array([(a[i, 0] * v[0] + a[i, 1] * v[1]) + a[i, 2] * v[2] for i in range(3)], np.float64)


def mul3(a, b):
    return np.array([[(a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j] for j in range(3)] for i in range(3)], np.float64)


def split(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return T[:3, :3].copy(), T[:3, 3].copy()


def rigid_inverse(R, t):
    """THE PROJECT'S RULE: (R, t)^-1 = (R^T, -(R^T t))"""
    Ri = np.ascontiguousarray(R.T)
    return Ri, -mulv(Ri, t)


def transform_f32(T, xyz):
    """pcl::transformPointCloud with a Matrix4d: f64, terms left to right, cast to f32"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(xyz, np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]).astype(np.float32) for i in range(3)], axis=1)


def voxel_of(w):
    """updateMap: (box triple i64, voxel centre i64, cell i64, key) of f32 world points"""
    x = np.asarray(w, np.float32).astype(np.float64)
    box = round_half_away(x * INV_VOXEL_RES)
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(box) < BOX_LIMIT, axis=1)  # (False for NaN)
    box = np.where(ok[:, None], box, 0.0).astype(np.int64)
    centre = np.trunc((box.astype(np.float64) * VOXEL_RES) * INV_POINT_RES).astype(np.int64)
    cell = np.trunc(np.where(ok[:, None], x, 0.0) * INV_POINT_RES).astype(np.int64)
    o = cell - centre + 5
    return ok, box, centre, cell, o[:, 0] * 100 + o[:, 1] * 10 + o[:, 2]


def u8_term(w, pix):
    """saturate_cast<uchar>(w * pix): cvRound (ties to even), saturated"""
    return int(min(max(np.rint(w * float(pix)), 0.0), 255.0))


def sample_bgr(img, row, col, margins=None):
    """getSubPixel<cv::Vec3b>(img, row, col): four u8 terms per channel, added left to right with saturation; a tap of weight zero is not read"""
    fr, fc = math.floor(row), math.floor(col)
    ar, ac = row - fr, col - fc
    w = [(1.0 - ar) * (1.0 - ac), ar * (1.0 - ac), (1.0 - ar) * ac, ar * ac]
    taps = [(fr, fc), (fr + 1, fc), (fr, fc + 1), (fr + 1, fc + 1)]
    out = [0, 0, 0]
    for wt, (r, c) in zip(w, taps):
        if wt == 0.0:
            continue
        for ch in range(3):
            t = wt * float(img[r, c, ch])
            if margins is not None:
                margins.append(abs((t - math.floor(t)) - 0.5))
            out[ch] = min(out[ch] + u8_term(wt, img[r, c, ch]), 255)
    return out


class Camera:
    """CameraModel / ImageRender: K read as f32, ext = (camera_extrinsic lidar_static^-1)^-1, setPose, project3DPoints, point2DAvailable"""

    def __init__(self, K4, extrinsic, lidar_static=None):
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(k)) for k in K4)
        Rl, tl = split(np.eye(4) if lidar_static is None else lidar_static)
        Rli, tli = rigid_inverse(Rl, tl)
        Re, te = split(extrinsic)
        Rs, ts = mul3(Re, Rli), mulv(Re, tli) + te
        self.Rx, self.tx = rigid_inverse(Rs, ts)
        self.R, self.t = np.eye(3), np.zeros(3)

    def set_pose(self, pose):
        Rp, tp = split(pose)
        Rw, tw = mul3(Rp, self.Rx), mulv(Rp, self.tx) + tp
        self.R, self.t = rigid_inverse(Rw, tw)

    def project(self, xyz):
        """(ok, u, v, z) of f64 points (n, 3)"""
        p = np.asarray(xyz, np.float64).reshape(-1, 3)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        R, t = self.R, self.t
        px = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
        py = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
        pz = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
        ok = ~(pz < 0.001) & ~np.isnan(pz)
        with np.errstate(all="ignore"):
            u = px * self.fx / pz + self.cx
            v = py * self.fy / pz + self.cy
        return ok, u, v, pz

    @staticmethod
    def available(cols, rows, u, v):
        with np.errstate(invalid="ignore"):
            return (u >= (MARGIN * cols + 1)) & (np.ceil(u) < ((1 - MARGIN) * cols)) & (v >= (MARGIN * rows + 1)) & (np.ceil(v) < ((1 - MARGIN) * rows))


def boundary_margin(cols, rows, u, v):
    """the smallest distance (px) of kept projections to a rounding boundary (fraction one half) or to an availability boundary"""
    if len(u) == 0:
        return np.inf
    m = np.inf
    for a, size in ((u, cols), (v, rows)):
        m = min(m, np.min(np.abs((a - np.floor(a)) - 0.5)))
        m = min(m, np.min(np.abs(a - (MARGIN * size + 1))))
        m = min(m, np.min(np.abs(a - (math.ceil((1 - MARGIN) * size) - 1))))
    return float(m)


# ---- the painter --------------------------------------------------------------------------------------------------------------------------
class Painter:
    """MapRender: setParameter, render (gate, insert, per-image projection / z-buffer / continuity / blend), getColorMap"""

    def __init__(self, cameras, lidar_static=None, active=True):
        self.cams = {str(n): Camera(K, E, lidar_static) for n, (K, E) in cameras.items()}
        self.active = active
        self.last_pose = np.eye(4)
        self.clear()
        self.stats = dict(rejected_same_cell=0, rejected_other_cell=0, gated=0, masked=0, losers=0, serial_ties=0, discontinuous=0, low_score=0, too_deep=0,
                          two_cameras=0, skipped=0, no_floor=0, rendered=0, min_boundary_margin=np.inf, min_term_margin=np.inf, blended=0)
        self.last_image = None

    def clear(self):
        self.vox_id = {}      # box triple -> voxel number
        self.box, self.centre, self.hits = [], [], []
        self.vkeys = []       # per voxel: key -> cell triple of the point that holds it
        self.vpts = []        # per voxel: serial numbers
        self.pos, self.vox, self.rgb, self.score, self.depth = [], [], [], [], []

    def moved(self, pose):
        Rl, tl = split(self.last_pose)
        Rli, tli = rigid_inverse(Rl, tl)
        d = mulv(Rli, split(pose)[1]) + tli
        return not (math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < MIN_MOVE)

    def insert(self, w):
        ok, box, centre, cell, key = voxel_of(w)
        touched = set()
        for i in range(len(w)):
            if not ok[i]:
                continue
            b = (int(box[i, 0]), int(box[i, 1]), int(box[i, 2]))
            v = self.vox_id.get(b)
            if v is None:
                v = self.vox_id[b] = len(self.box)
                self.box.append(b)
                self.centre.append(tuple(int(c) for c in centre[i]))
                self.hits.append(0)
                self.vkeys.append({})
                self.vpts.append([])
            touched.add(v)
            k, c = int(key[i]), tuple(int(x) for x in cell[i])
            held = self.vkeys[v].get(k)
            if held is None:
                self.vkeys[v][k] = c
                self.vpts[v].append(len(self.pos))
                self.pos.append(np.asarray(w[i], np.float32))
                self.vox.append(v)
                self.rgb.append(np.zeros(3, np.float32))
                self.score.append(np.float32(0))
                self.depth.append(np.float32(100.0))
            else:
                self.stats["rejected_same_cell" if held == c else "rejected_other_cell"] += 1
        hits = sorted(touched)
        for v in hits:
            self.hits[v] += 1
        return hits

    def paint(self, cam, img, hits):
        rows, cols = img.shape[:2]
        st = self.stats
        cs, cu, cv, cz = [], [], [], []
        for v in hits:
            c = np.array(self.centre[v], np.float64) * POINT_RES
            ok, u, vv, z = cam.project(c[None])
            if not (ok[0] and cam.available(cols, rows, u, vv)[0] and not (z[0] <= MIN_DEPTH) and not (z[0] >= MAX_DEPTH)):
                st["gated"] += 1
                continue
            ser = np.array(self.vpts[v], np.int64)
            ok, pu, pv, pz = cam.project(np.array([self.pos[s] for s in ser], np.float32).astype(np.float64))
            kept = ok & cam.available(cols, rows, pu, pv)
            ku, kv = pu[kept], pv[kept]
            st["min_boundary_margin"] = min(st["min_boundary_margin"], boundary_margin(cols, rows, ku, kv))
            umax, umin = max(u[0], ku.max(initial=-np.inf)), min(u[0], ku.min(initial=np.inf))
            vmax, vmin = max(vv[0], kv.max(initial=-np.inf)), min(vv[0], kv.min(initial=np.inf))
            if (umax - umin) <= 10.0 and (vmax - vmin) <= 10.0:
                st["masked"] += 1
                continue
            cs.append(ser[kept]); cu.append(ku); cv.append(kv); cz.append(pz[kept])
        depth = np.full(rows * cols, -1.0, np.float32)
        owner = np.full(rows * cols, -1, np.int32)
        valid = np.zeros(rows * cols, np.uint8)
        self.last_image = dict(depth=depth.reshape(rows, cols), owner=owner.reshape(rows, cols), valid=valid.reshape(rows, cols))
        if not cs:
            return []
        ser, u, v, z = np.concatenate(cs), np.concatenate(cu), np.concatenate(cv), np.concatenate(cz)
        zf = z.astype(np.float32)
        pix = round_half_away(v).astype(np.int64) * cols + round_half_away(u).astype(np.int64)
        order = np.lexsort((ser, zf, pix))  # per pixel: the smallest (float)z, ties to the smaller serial number
        first = np.ones(len(order), bool)
        first[1:] = pix[order][1:] != pix[order][:-1]
        win = order[first]
        st["losers"] += len(order) - len(win)
        second = order[1:][~first[1:]]  # runners-up and beyond; a tie when one shares pixel and depth with its predecessor
        prev = order[:-1][~first[1:]]
        st["serial_ties"] += int(np.sum(zf[second] == zf[prev]))
        depth[pix[win]] = zf[win]
        owner[pix[win]] = ser[win]
        # checkDepthContinuous: the window is centred on the TRUNCATED position
        dmin, dmax = zf[win].copy(), zf[win].copy()
        d2 = depth.reshape(rows, cols)
        for i in range(-4, 5):
            iu = (u[win] + i).astype(np.int64)  # (int) truncates toward zero
            for j in range(-4, 5):
                jv = (v[win] + j).astype(np.int64)
                inside = (iu >= 0) & (iu < cols) & (jv >= 0) & (jv < rows)
                d = d2[np.clip(jv, 0, rows - 1), np.clip(iu, 0, cols - 1)]
                use = inside & ~(d < 0)
                dmin = np.where(use, np.minimum(dmin, d), dmin)
                dmax = np.where(use, np.maximum(dmax, d), dmax)
        good = ~((dmax - dmin).astype(np.float64) > 2.0)
        st["discontinuous"] += int(np.sum(~good))
        valid[pix[win]] = good
        painted = []
        margins = []
        for k in win[good]:
            s = int(ser[k])
            score = np.float32(1.0 - abs(u[k] - cols / 2.0) / (cols / 2.0))
            if float(score) < 0.1:
                st["low_score"] += 1
                continue
            if z[k] > float(self.depth[s]) * 1.5:
                st["too_deep"] += 1
                continue
            if z[k] < float(self.depth[s]):
                self.depth[s] = np.float32(z[k])
            bgr = sample_bgr(img, float(v[k]), float(u[k]), margins)
            s1, s2 = float(self.score[s]), float(score)
            rgb = self.rgb[s]
            self.rgb[s] = np.array([np.float32((float(rgb[c]) * s1 + float(bgr[2 - c]) * s2) / (s1 + s2)) for c in range(3)], np.float32)
            self.score[s] = np.float32(max(s1, s2))
            painted.append(s)
        if margins:
            st["min_term_margin"] = min(st["min_term_margin"], min(margins))
        st["blended"] += len(painted)
        return painted

    def frame(self, xyzi, pose, images=None, ground=None):
        """render(pose, frame, images); ground: None (the points as they are) or a callable frame -> floor inliers or None"""
        pose = np.asarray(pose, np.float64).reshape(4, 4)
        images = images or {}
        for img, _ in images.values():
            if np.asarray(img).ndim != 3:
                raise ValueError("an image must be rows x cols x 3 (BGR)")
        if not self.active or not self.moved(pose):
            self.stats["skipped"] += 1
            return "skipped"
        self.last_pose = pose.copy()
        pts = np.asarray(xyzi, np.float32).reshape(-1, 4)
        if ground is not None:
            pts = ground(pts)
            if pts is None:
                self.stats["no_floor"] += 1
                return "no_floor"
        hits = self.insert(transform_f32(pose, pts[:, :3]))
        seen = {}
        for name in sorted(images):
            img, ipose = images[name]
            cam = self.cams[str(name)]
            cam.set_pose(ipose)
            for s in self.paint(cam, np.asarray(img, np.uint8), hits):
                seen[s] = seen.get(s, 0) + 1
        self.stats["two_cameras"] += sum(1 for c in seen.values() if c > 1)
        self.stats["rendered"] += 1
        return "rendered"

    def colour_map(self):
        """getColorMap + pointcloud_to_numpy(PointCloudRGB): ascending voxel number, then serial number"""
        rows = []
        for v in range(len(self.box)):
            if self.hits[v] <= 2:
                continue
            for s in self.vpts[v]:
                if float(self.score[s]) < 0.1:
                    continue
                r, g, b = (int(np.uint8(int(c))) for c in self.rgb[s])
                rows.append((self.pos[s], np.uint32(r << 16 | g << 8 | b)))
        out = np.zeros((len(rows), 4), np.float32)
        for i, (p, w) in enumerate(rows):
            out[i, :3] = p
            out[i, 3:].view(np.uint32)[0] = w
        return out

    def state(self):
        n = len(self.pos)
        return dict(box=np.array(self.box, np.int32).reshape(-1, 3), hits=np.array(self.hits, np.uint32), counts=np.array([len(p) for p in self.vpts], np.uint32),
                    xyz=np.array(self.pos, np.float32).reshape(n, 3), voxel=np.array(self.vox, np.uint32), rgb=np.array(self.rgb, np.float32).reshape(n, 3),
                    score=np.array(self.score, np.float32), depth=np.array(self.depth, np.float32))


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def se3(R=None, t=(0, 0, 0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


CAM_AXES = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])  # camera (x right, y down, z forward) in the body (x forward, y left, z up)


def mount(yaw=0.0, pitch=20.0, t=(0.5, 0.0, 0.5)):
    """the camera_extrinsic of a camera mounted at t in the lidar frame, looking forward, pitched down: the inverse of its pose in that frame"""
    return np.linalg.inv(se3(rot("z", yaw) @ rot("y", pitch) @ CAM_AXES, t))


def image(rows, cols, seed):
    """a smooth gradient plus noise, BGR u8"""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:rows, 0:cols]
    base = np.stack([40 + 150 * c / cols, 30 + 180 * r / rows, 200 - 120 * (r + c) / (rows + cols)], axis=2)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def world_scene(seed, n_floor, n_wall, x_range=(0.5, 8.5), y_range=(-2.0, 2.0), floor_z=-1.0):
    """world-fixed points: a floor patch at floor_z and a box standing on it (near face and top), f32"""
    rng = np.random.default_rng(seed)
    fl = np.stack([rng.uniform(*x_range, n_floor), rng.uniform(*y_range, n_floor), floor_z + rng.normal(0, 0.004, n_floor)], axis=1)
    face = np.stack([np.full(n_wall, 4.3) + rng.normal(0, 0.003, n_wall), rng.uniform(-0.6, 0.6, n_wall), rng.uniform(floor_z, floor_z + 0.7, n_wall)], axis=1)
    top = np.stack([rng.uniform(4.3, 4.7, n_wall // 2), rng.uniform(-0.6, 0.6, n_wall // 2), np.full(n_wall // 2, floor_z + 0.7)], axis=1)
    return np.concatenate([fl, face, top]).astype(np.float32)


def body_frame(world, pose, x_window):
    """what the sensor at `pose` sees of the world points: those whose body x lies in the window, in the body frame, with an intensity column"""
    R, t = split(pose)
    b = (world.astype(np.float64) - t) @ R  # R^T (p - t)
    keep = (b[:, 0] >= x_window[0]) & (b[:, 0] < x_window[1])
    out = np.zeros((int(keep.sum()), 4), np.float32)
    out[:, :3] = b[keep]
    out[:, 3] = 0.5
    return out


def _drive(xs, yaw=0.0):
    return [se3(rot("z", yaw * x), (x, 0.02 * x, 0.0)) for x in xs]


def _kernel_case(seed, cams, lidar_static, yaw, rows=240, cols=320, n_floor=6000):
    world = world_scene(seed, n_floor, 300)
    # the first pose is the identity (dropped by the gate: last_pose starts there), one later pose moves 5 cm (dropped too)
    xs = [0.0, 0.3, 0.6, 0.65, 0.9, 1.2, 1.5]
    frames = []
    for k, pose in enumerate(_drive(xs, yaw)):
        images = {name: (image(rows, cols, 1000 * seed + 10 * k + j), pose) for j, name in enumerate(sorted(cams))}
        frames.append(dict(points=body_frame(world, pose, (1.0, 5.5)), pose=pose, images=images))
    return dict(cameras=cams, lidar_static=lidar_static, frames=frames, ground=False, max_voxels=4096, max_points=1 << 16)


def _integer_case():
    """160 x 120, a camera 4 m above the floor looking straight down with f = 256: u = 64 (x - px) + 80 and v = -64 (y - py) + 60 exactly, so
    points on the 1/16 m lattice land on integer pixels (three of the four taps have weight zero; edge_tap_case has one on the last available row
    and column, where the reference's fourth tap lies outside the image).  Partners a fifth of a pixel away share a pixel with them at the same
    f32 depth."""
    E = np.linalg.inv(se3(np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, 4.0)))
    cams = {"down": ((256.0, 256.0, 80.0, 60.0), E)}
    pts = []
    for i in range(-19, 20):
        for j in range(-14, 15):
            pts.append((i / 16.0, j / 16.0, 0.0))
    lattice = len(pts)
    rng = np.random.default_rng(5)
    for i, j in rng.integers(-15, 15, (150, 2)):  # partners a fifth of a pixel away, some of them 1e-8 m higher: the f64 depths differ, the f32 do not
        pts.append((i / 16.0 + 0.003, j / 16.0 - 0.002, 1e-8 if (i + j) % 2 else 0.0))
    for x, y in rng.uniform(-1.1, 1.1, (600, 2)):
        pts.append((x, y, 0.0))
    world = np.zeros((len(pts), 4), np.float32)
    world[:, :3] = np.array(pts, np.float32)
    frames = []
    for k, px in enumerate([0.0, 0.3125, 0.625, 0.9375, 1.25]):
        pose = se3(None, (px, 0.0, 0.0))
        body = world.copy()
        body[:, 0] = (world[:, 0].astype(np.float64) - px).astype(np.float32)  # (exact for the lattice: multiples of 1/16 below 4)
        frames.append(dict(points=body, pose=pose, images={"down": (image(120, 160, 77 + k), pose)}))
    return dict(cameras=cams, lidar_static=None, frames=frames, ground=False, max_voxels=4096, max_points=1 << 16, lattice=lattice)


def edge_tap_case():
    """one frame under the camera of integer_pixels, standing at (63/64, -11/64): the point (83/64, -70/64, 0) lands on u = 100, v = 119 exactly,
    the last available row of a 160 x 120 image, where ceil = floor + 1 names a row outside it (on the last column, 159, the score is below 0.1
    and nothing is sampled).  The other points spread
    its voxel over more than 10 px.  The point sits ON the availability boundary by construction (exact arithmetic), so the case is kept apart
    from those whose margins are checked."""
    c = _integer_case()
    rng = np.random.default_rng(9)
    pts = [(83.0 / 64.0, -70.0 / 64.0, 0.0)] + [(83.0 / 64.0 - a, -70.0 / 64.0 + b, 0.0) for a, b in rng.uniform(0.0, 0.18, (40, 2))]
    body = np.zeros((len(pts), 4), np.float32)
    body[:, :3] = np.array(pts, np.float32)
    body[:, 0] = (body[:, 0].astype(np.float64) - 0.3125).astype(np.float32)
    frame = dict(points=body, pose=se3(None, (0.3125, 0.0, 0.0)), images={"down": (image(120, 160, 123), se3(None, (0.984375, -0.171875, 0.0)))})
    return dict(cameras=c["cameras"], lidar_static=None, frames=[frame], ground=False, max_voxels=256, max_points=4096)


def _ground_case():
    """about 3 000 floor points plus clutter through the ground test; one frame of clutter alone has no floor"""
    rng = np.random.default_rng(11)
    world = world_scene(11, 5200, 200, x_range=(0.5, 7.5))
    clutter = np.stack([rng.uniform(1, 6, 500), rng.uniform(-2, 2, 500), rng.uniform(0.3, 1.4, 500)], axis=1).astype(np.float32)
    cams = {"front": ((300.0, 300.0, 160.0, 120.0), mount())}
    frames = []
    for k, pose in enumerate(_drive([0.3, 0.6, 0.9, 1.2, 1.5])):
        pts = body_frame(np.concatenate([world, clutter + pose[:3, 3].astype(np.float32)]), pose, (1.0, 5.5))
        if k == 2:  # nothing near the floor: detect_ground returns none
            pts = body_frame(clutter + pose[:3, 3].astype(np.float32), pose, (1.0, 5.5))
        frames.append(dict(points=pts, pose=pose, images={"front": (image(240, 320, 300 + k), pose)}, seed=40 + k))
    return dict(cameras=cams, lidar_static=None, frames=frames, ground=True, max_voxels=4096, max_points=1 << 16)


K = (300.0, 300.0, 160.0, 120.0)
CASE_NAMES = ["one_camera", "two_cameras", "three_cameras_static", "integer_pixels", "ground"]
KERNEL_CASES = CASE_NAMES[:4]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "one_camera":
        return _kernel_case(1, {"front": (K, mount())}, None, 0.0)
    if name == "two_cameras":
        # "rear" sits 3 m behind "front" and comes later in name order: what front paints at depth d it sees beyond 1.5 d
        return _kernel_case(2, {"front": (K, mount()), "rear": ((310.0, 305.0, 158.5, 121.25), mount(t=(-2.5, 0.1, 0.6), pitch=12.0))}, None, 1.5)
    if name == "three_cameras_static":
        ls = se3(rot("z", 2.0) @ rot("x", 0.5), (0.1, -0.05, 0.02))
        return _kernel_case(4, {"a_left": (K, mount(yaw=18.0)), "b_mid": (K, mount()), "c_right": ((295.0, 301.0, 161.0, 119.0), mount(yaw=-18.0))}, ls, -1.0,
                            n_floor=5000)
    if name == "integer_pixels":
        return _integer_case()
    if name == "ground":
        return _ground_case()
    raise KeyError(name)


def run(name, ground=None):
    """the case through the restatement: (painter, outcomes); `ground` as Painter.frame takes it (per frame: called with the frame's seed).
    painter.snapshots holds, per frame, the z-buffer of its last image (None for a frame that was not rendered) and the map's size."""
    c = case(name) if isinstance(name, str) else name
    p = Painter(c["cameras"], c["lidar_static"])
    out, p.snapshots = [], []
    for f in c["frames"]:
        g = None
        if c["ground"]:
            g = functools.partial(ground, seed=f.get("seed", 0))
        out.append(p.frame(f["points"], f["pose"], f["images"], g))
        img = {k: v.copy() for k, v in p.last_image.items()} if out[-1] == "rendered" and f["images"] else None
        p.snapshots.append(dict(image=img, size=(len(p.box), len(p.pos))))
    return p, out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the kernel cases' restated result, computed once and shared by the tests (do not modify)"""
    assert name in KERNEL_CASES
    return run(name)
