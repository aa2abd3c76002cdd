"""Host-side objects over the C ABI: Map (iVox), Scan (per-scan buffers) and Engine (fastlio_main body).

Names and argument meaning follow the reference's FastLIO frontend
(/root/reference/slam/mapping/fastlio/src/laserMapping.cpp): `Engine.process_scan` is the part of
`fastlio_main()` that follows IMU processing, `Engine.update` is
`kf.update_iterated_dyn_share_modified(LASER_POINT_COV)`, `Map.add` is `ivox->AddPoints`,
`Map.knn` is `ivox->GetClosestPoint(p, out, 5, 5.0)`, `Scan.voxel_downsample` is `downSizeFilterSurf.filter`.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import check, f32, f64, lib, ptr

STATE_DIM = 26  # pos3 rot4(xyzw) R_il4 t_il3 vel3 bg3 ba3 grav3  (use-ikfom.hpp:12-21)
DOF = 23
G_LEN = 9.809


def default_state():
    s = np.zeros(STATE_DIM)
    s[6] = 1.0
    s[10] = 1.0
    s[23] = G_LEN
    return s


def init_cov():
    """covariance after IMU initialisation (IMU_Processing.hpp:224-231)"""
    P = np.eye(23)
    for i in (6, 7, 8, 9, 10, 11):
        P[i, i] = 0.00001
    for i in (15, 16, 17):
        P[i, i] = 0.0001
    for i in (18, 19, 20):
        P[i, i] = 0.001
    P[21, 21] = P[22, 22] = 0.00001
    return P


def _pose_ext(state):
    s = f64(state)
    pose = np.concatenate([s[0:3], s[3:7]])
    ext = np.concatenate([s[11:14], s[7:11]])
    return f64(pose), f64(ext)


class Map:
    def __init__(self, resolution=0.5, stencil=19, max_points=2_000_000, max_voxels=1_000_000, device=0, _borrow=None):
        self._own = _borrow is None
        self.h = _borrow if _borrow is not None else lib().lio_map_create(device, resolution, max_points, max_voxels, stencil)
        if not self.h:
            raise capi.LioError("lio_map_create failed: " + lib().lio_last_error().decode())

    def set_lru(self, capacity_voxels, max_distance=100.0):
        """IVox capacity_ / max_distance_: least-recently-touched voxels are dropped above `capacity_voxels` (call before the first add)"""
        check(lib().lio_map_set_lru(self.h, int(capacity_voxels), float(max_distance)), "set_lru")

    def lru_stats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib().lio_map_lru_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def lru_exact_stats(self):
        """(voxels dropped and re-created inside a batch as the reference's point-by-point order does, batches in which that order was not followed)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib().lio_map_lru_exact_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def clear(self):
        """back to an empty map (memory kept)"""
        check(lib().lio_map_clear(self.h), "map clear")

    def set_tie_mode(self, mode):
        """1 (default): candidates exactly as far as the fifth nearest are kept as the reference's std::nth_element keeps them; 0: smallest (d2, x, y, z);
        2: the lists exactly as the reference returns them, order included (every query redone by the reference's selection: slow, a parity mode)"""
        check(lib().lio_map_set_tie_mode(self.h, int(mode)), "set_tie_mode")

    def tie_stats(self):
        """(queries whose neighbour set the reference's selection decided, those of them left unresolved)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib().lio_map_tie_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pool_stats(self):
        top, cap = C.c_uint64(), C.c_uint64()
        check(lib().lio_map_pool_stats(self.h, C.byref(top), C.byref(cap)), "pool stats")
        return top.value, cap.value

    def close(self):
        if getattr(self, "h", None) and self._own and lib is not None:  # `lib` is gone at interpreter shutdown
            lib().lio_map_destroy(self.h)
        self.h = None

    __del__ = close

    def set_stencil(self, s):
        check(lib().lio_map_set_stencil(self.h, s), "set_stencil")

    def add(self, pts, travel=0.0):
        p = f32(pts).reshape(-1, 4)
        check(lib().lio_map_insert(self.h, ptr(p, C.c_float), len(p), float(travel)), "map insert")

    def add_device(self, dptr, n, travel=0.0):
        check(lib().lio_map_insert_device(self.h, C.c_void_p(dptr), n, float(travel)), "map insert (device)")

    def stats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib().lio_map_stats(self.h, C.byref(a), C.byref(b)), "map stats")
        return int(a.value), int(b.value)

    @property
    def num_points(self):
        return self.stats()[0]

    @property
    def num_voxels(self):
        return self.stats()[1]

    @property
    def nbytes(self):
        return int(lib().lio_map_bytes(self.h))

    @property
    def knn_candidates(self):
        return int(lib().lio_map_knn_candidates(self.h))

    @property
    def knn_unique(self):
        """distinct points per launch the kNN sweep loaded, summed over the counted launches (diagnostic kernel variant only)"""
        return int(lib().lio_map_knn_unique(self.h))

    @property
    def knn_touched(self):
        """points the kNN sweep loaded so far (counted by the diagnostic kernel variant only: Batch.enable_kernel_timing(2))"""
        return int(lib().lio_map_knn_touched(self.h))

    def dump(self):
        n = self.num_points
        out = np.zeros((max(n, 1), 4), np.float32)
        m = check(lib().lio_map_dump(self.h, ptr(out, C.c_float), max(n, 1)), "map dump")
        return out[:m]

    def knn(self, q):
        q = f32(q).reshape(-1, 4)
        out = np.zeros((len(q), 5, 4), np.float32)
        cnt = np.zeros(len(q), np.int32)
        check(lib().lio_map_knn(self.h, ptr(q, C.c_float), len(q), ptr(out, C.c_float), ptr(cnt, C.c_int32)), "map knn")
        return out, cnt


class Scan:
    def __init__(self, max_raw=262144, max_ds=100000, device=0, _borrow=None):
        self._own = _borrow is None
        self.max_ds = max_ds
        self.h = _borrow if _borrow is not None else lib().lio_scan_create(device, max_raw, max_ds)
        if not self.h:
            raise capi.LioError("lio_scan_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and self._own and lib is not None:
            lib().lio_scan_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self):
        check(lib().lio_scan_reset(self.h), "scan reset")

    def upload(self, body_xyzi):
        p = f32(body_xyzi).reshape(-1, 4)
        check(lib().lio_scan_upload(self.h, ptr(p, C.c_float), len(p)), "scan upload")
        self._keep = p

    def set_device(self, dptr, n):
        check(lib().lio_scan_set_device(self.h, C.c_void_p(dptr), n), "scan set_device")

    def undistort_delta(self, stamp_us, delta_pose, scan_period=0.1, on_device=False):
        """undistortPoints(delta_pose, points, scan_period) of the localisation mode (slam_utils.cpp:163-191) on the uploaded cloud;
        stamp_us: host uint32 array, or a device pointer with on_device=True"""
        d = np.ascontiguousarray(delta_pose, np.float32).reshape(16)
        if on_device:
            sp = C.c_void_p(int(stamp_us))
        else:
            self._stamps = np.ascontiguousarray(stamp_us, np.uint32)
            sp = C.c_void_p(self._stamps.ctypes.data)
        check(lib().lio_scan_undistort_delta(self.h, sp, int(on_device), d.ctypes.data_as(C.POINTER(C.c_float)), float(scan_period)), "undistort_delta")

    def undistort_poses(self, stamp_us, header_stamp_us, pose_stamps_us, pose_T):
        """undistortPoints(poses, points) of slam_utils.cpp:193-228 on the uploaded cloud (host stamps)"""
        self._stamps = np.ascontiguousarray(stamp_us, np.uint32)
        ps, pt = np.ascontiguousarray(pose_stamps_us, np.uint64), np.ascontiguousarray(pose_T, np.float64).reshape(-1, 16)
        check(lib().lio_scan_undistort_poses(self.h, C.c_void_p(self._stamps.ctypes.data), 0, int(header_stamp_us), ps.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             pt.ctypes.data_as(C.POINTER(C.c_double)), len(ps)), "undistort_poses")

    def undistort_imu(self, stamp_us, poses, end_pos, end_rot_xyzw, ril_xyzw, til, blind=0.1, filter_num=1, undistort=True):
        """the FastLIO front half's point filter and IMU backward propagation (IMU_Processing.hpp:371-404) on the uploaded cloud with the
        caller's poses: rows of 22 doubles (offset s, acc, gyr, vel, pos, R row-major); host stamps.  Dropped points come back NaN."""
        self._stamps = np.ascontiguousarray(stamp_us, np.uint32)
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 22)
        a = [np.ascontiguousarray(v, np.float64).reshape(k) for v, k in ((end_pos, 3), (end_rot_xyzw, 4), (ril_xyzw, 4), (til, 3))]
        check(lib().lio_scan_undistort_imu(self.h, C.c_void_p(self._stamps.ctypes.data), 0, ptr(P, C.c_double), len(P), *[ptr(v, C.c_double) for v in a],
                                           float(blind), int(filter_num), int(bool(undistort))), "undistort_imu")

    def download_raw(self, cap=1 << 18):
        out = np.zeros((cap, 4), np.float32)
        n = lib().lio_scan_download_raw(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), cap)
        if n < 0:
            check(n, "download_raw")
        return out[:n].copy()

    def voxel_downsample(self, leaf=0.5, sync=True):
        n = C.c_uint32(0)
        check(lib().lio_scan_voxel_downsample(self.h, float(leaf), int(sync), C.byref(n)), "voxel downsample")
        return int(n.value)

    @staticmethod
    def voxel_downsample_batch(scans, leaf=0.5):
        """lio_scan_voxel_downsample_batch: the VoxelGrid of many scans with one set of launches; returns the point counts"""
        hs = (C.c_void_p * len(scans))(*[s.h for s in scans])
        n = (C.c_uint32 * len(scans))()
        check(lib().lio_scan_voxel_downsample_batch(hs, len(scans), float(leaf), n), "voxel downsample batch")
        return [int(v) for v in n]

    def set_ds(self, ds):
        d = f32(ds).reshape(-1, 4)
        check(lib().lio_scan_set_ds(self.h, ptr(d, C.c_float), len(d)), "set_ds")

    @property
    def num_ds(self):
        return check(lib().lio_scan_num_ds(self.h), "num_ds")

    def get_ds(self):
        out = np.zeros((self.max_ds, 4), np.float32)
        n = check(lib().lio_scan_download_ds(self.h, ptr(out, C.c_float), self.max_ds), "download ds")
        return out[:n].copy()

    def get_world(self):
        out = np.zeros((self.max_ds, 4), np.float32)
        n = check(lib().lio_scan_download_world(self.h, ptr(out, C.c_float), self.max_ds), "download world")
        return out[:n].copy()

    def set_degeneracy_mode(self, mode):
        """0 auto (bound-gated), 1 always evaluate, 2 never"""
        check(lib().lio_scan_set_degeneracy_mode(self.h, int(mode)))

    def degeneracy(self, V):
        V = f64(V).reshape(3, 3)
        c, s_ = np.zeros(3), np.zeros(3)
        check(lib().lio_p2plane_degeneracy(self.h, ptr(V, C.c_double), ptr(c, C.c_double), ptr(s_, C.c_double)), "degeneracy")
        return c, s_

    def enable_kernel_timing(self, mask=3):
        """bit mask: 1 = kNN kernel, 2 = linearize kernel, 0 = off"""
        check(lib().lio_scan_enable_kernel_timing(self.h, int(mask)))

    def kernel_times(self, reset=True):
        t = capi.KernelTimes()
        check(lib().lio_scan_kernel_times(self.h, C.byref(t), int(reset)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "pad"}

    def get_match(self):
        n = self.num_ds
        sel = np.zeros(n, np.uint8)
        nv = np.zeros((n, 4), np.float32)
        cnt = np.zeros(n, np.int32)
        nn = np.zeros((n, 5, 4), np.float32)
        check(lib().lio_scan_download_match(self.h, ptr(sel, C.c_uint8), ptr(nv, C.c_float), ptr(cnt, C.c_int32), ptr(nn, C.c_float)),
              "download match")
        return dict(selected=sel, normvec=nv, nn_cnt=cnt, nn=nn)


def linearize(map_, scan, state, redo_knn=True):
    """one evaluation of h_share_model_geometric at `state` (26 doubles); returns the normal equations"""
    pose, ext = _pose_ext(state)
    ne = capi.NormalEq()
    check(lib().lio_p2plane_linearize(map_.h, scan.h, ptr(pose, C.c_double), ptr(ext, C.c_double), int(redo_knn), C.byref(ne)), "linearize")
    return dict(n_eff=int(ne.n_eff), n_ds=int(ne.n_ds), JtJ=np.array(ne.JtJ).reshape(6, 6), Jtr=np.array(ne.Jtr),
                nnT=np.array(ne.nnT).reshape(3, 3), eigvec=np.array(ne.eigvec).reshape(3, 3), eigval=np.array(ne.eigval),
                contri=np.array(ne.contri), strong=np.array(ne.strong), sum_abs_res=float(ne.sum_abs_res), n_tie=int(ne.n_tie),
                knn_candidates=(int(ne.n_knn_candidates_hi) << 32) | int(ne.n_knn_candidates_lo))


def map_incremental(map_, scan, state, map_leaf=0.5, ekf_inited=True, travel=0.0):
    pose, ext = _pose_ext(state)
    return check(lib().lio_map_incremental(map_.h, scan.h, ptr(pose, C.c_double), ptr(ext, C.c_double), float(map_leaf), int(ekf_inited),
                                           float(travel)), "map_incremental")


class Engine:
    """The FastLIO per-scan engine (state + covariance + map + scan buffers) on one GPU."""

    def __init__(self, resolution=0.5, stencil=75, max_points=2_000_000, max_voxels=1_000_000, max_raw=262144, max_ds=100000, device=0,
                 shared_map=None):
        if shared_map is not None:  # read-only engine on somebody else's map (several may run concurrently)
            self._shared = shared_map
            self.h = lib().lio_engine_create_shared(shared_map.h, max_raw, max_ds)
        else:
            self.h = lib().lio_engine_create(device, resolution, stencil, max_points, max_voxels, max_raw, max_ds)
        if not self.h:
            raise capi.LioError("lio_engine_create failed: " + lib().lio_last_error().decode())
        self.map = Map(_borrow=lib().lio_engine_map(self.h))
        self.scan = Scan(max_ds=max_ds, _borrow=lib().lio_engine_scan(self.h))

    def close(self):
        if getattr(self, "h", None) and getattr(self, "_own", True) and lib is not None:
            lib().lio_engine_destroy(self.h)
        self.h = None

    __del__ = close

    def set_device_loop(self, on=True):
        """run the iterate loop of this engine's updates on the device (one submission, one wait) instead of from the host"""
        check(lib().lio_engine_set_device_loop(self.h, int(on)), "set_device_loop")

    def set_state(self, s):
        s = f64(s)
        assert s.size == STATE_DIM
        check(lib().lio_engine_set_state(self.h, ptr(s, C.c_double)))

    def get_state(self):
        s = np.zeros(STATE_DIM)
        check(lib().lio_engine_get_state(self.h, ptr(s, C.c_double)))
        return s

    def set_cov(self, P):
        P = f64(P).reshape(23, 23)
        check(lib().lio_engine_set_cov(self.h, ptr(P, C.c_double)))

    def get_cov(self):
        P = np.zeros((23, 23))
        check(lib().lio_engine_get_cov(self.h, ptr(P, C.c_double)))
        return P

    def set_flags(self, ekf_inited=True, first_scan=False, travel=0.0, first_lidar_time=0.0):
        check(lib().lio_engine_set_flags(self.h, int(ekf_inited), int(first_scan), float(travel), float(first_lidar_time)))

    def set_stencil(self, s):
        self.map.set_stencil(s)

    def map_add(self, pts, travel=0.0):
        self.map.add(pts, travel)

    def set_ds(self, ds):
        self.scan.set_ds(ds)

    def get_ds(self):
        return self.scan.get_ds()

    def update(self):
        n = check(lib().lio_engine_update(self.h), "engine update")
        logs = []
        for i in range(n):
            pl = capi.PassLog()
            check(lib().lio_engine_pass_log(self.h, i, C.byref(pl)))
            logs.append(dict(knn=pl.knn, n_eff=pl.n_eff, valid=pl.valid, degenerate=pl.degenerate, sum_abs_res=pl.sum_abs_res,
                             JtJ=np.array(pl.JtJ).reshape(6, 6), Jtr=np.array(pl.Jtr), dx=np.array(pl.dx)))
        return logs

    def map_incremental(self, map_leaf=0.5, ekf_inited=True):
        return map_incremental(self.map, self.scan, self.get_state(), map_leaf, ekf_inited, self.travel)

    def process_scan(self, raw, lidar_beg_time):
        r = f32(raw).reshape(-1, 4)
        return check(lib().lio_engine_process_scan(self.h, ptr(r, C.c_float), len(r), float(lidar_beg_time)), "process_scan")

    def process_scan_device(self, dptr, n, lidar_beg_time):
        return check(lib().lio_engine_process_scan_device(self.h, C.c_void_p(dptr), n, float(lidar_beg_time)), "process_scan")

    def enable_timing(self, on=True):
        check(lib().lio_engine_enable_timing(self.h, int(on)))

    # ---- the IMU front half: fastlio_init / _imu_enqueue / _pcl_enqueue / _main / _odometry / _state
    # (reference: slam/mapping/fastlio/src/laserMapping.cpp:1025,397,311,1126,692,714) ----
    def fastlio_init(self, extT=(0.0, 0.0, 0.0), extR=np.eye(3), filter_num=1, max_point_num=-1, scan_period=0.1, undistort=True):
        t, r = f64(extT), f64(extR).reshape(-1)
        assert t.size == 3 and r.size == 9
        check(lib().lio_fastlio_init(self.h, ptr(t, C.c_double), ptr(r, C.c_double), filter_num, max_point_num, float(scan_period), int(undistort)))

    def fastlio_is_init(self):
        return bool(lib().lio_fastlio_is_init(self.h))

    def fastlio_imu_enqueue(self, stamp, gyr, acc_ms2):
        g, a = f64(gyr), f64(acc_ms2)
        check(lib().lio_fastlio_imu_enqueue(self.h, float(stamp), ptr(g, C.c_double), ptr(a, C.c_double)))

    def fastlio_set_wheelspeed(self, on=True):
        """wheelspeed_en of laserMapping.cpp:83: append the wheel-speed rows (:794-811) when the scan's last INS sample is within 10 ms of its end"""
        check(lib().lio_fastlio_set_wheelspeed(self.h, int(on)), "set_wheelspeed")

    def fastlio_ins_enqueue(self, stamp, vel_imu):
        v = f64(vel_imu)
        check(lib().lio_fastlio_ins_enqueue(self.h, float(stamp), ptr(v, C.c_double)))

    def fastlio_pcl_enqueue(self, xyzi, stamp_us, header_stamp):
        p = f32(xyzi).reshape(-1, 4)
        t = np.ascontiguousarray(stamp_us, np.uint32)
        assert len(t) == len(p)
        check(lib().lio_fastlio_pcl_enqueue(self.h, ptr(p, C.c_float), ptr(t, C.c_uint32), len(p), float(header_stamp)))

    def fastlio_pcl_enqueue_device(self, d_xyzi, d_stamp_us, n, header_stamp):
        check(lib().lio_fastlio_pcl_enqueue_device(self.h, C.c_void_p(d_xyzi), C.c_void_p(d_stamp_us), n, float(header_stamp)))

    def fastlio_main(self):
        """one fastlio_main pass; returns capi MAIN_* (IDLE when there was nothing to do)"""
        return check(lib().lio_fastlio_main(self.h), "fastlio_main")

    def fastlio_odometry(self):
        a, b = np.zeros(16), np.zeros(16)
        check(lib().lio_fastlio_odometry(self.h, ptr(a, C.c_double), ptr(b, C.c_double)))
        return a.reshape(4, 4), b.reshape(4, 4)

    def fastlio_state(self):
        s = np.zeros(20)
        check(lib().lio_fastlio_state(self.h, ptr(s, C.c_double)))
        return s

    def fastlio_start_state(self):
        s = np.zeros(STATE_DIM)
        check(lib().lio_fastlio_start_state(self.h, ptr(s, C.c_double)))
        return s

    def undistorted(self, cap=300000):
        out = np.zeros((cap, 4), np.float32)
        n = C.c_uint32(0)
        check(lib().lio_fastlio_download_undistorted(self.h, ptr(out, C.c_float), cap, C.byref(n)))
        return out[:n.value].copy()


    def set_reduce_hook(self, fn):
        """fn(buf: np.ndarray) replaces the engine's local normal-equation sums by the global ones IN PLACE
        (see lsd_amd.dist.NormalEqAllGather); None removes the hook"""
        if fn is None:
            self._hook = None
            check(lib().lio_engine_set_reduce_hook(self.h, capi.REDUCE_FN(0), None))
            return

        def _cb(_ctx, p, n):
            fn(np.ctypeslib.as_array(p, shape=(n,)))

        self._hook = capi.REDUCE_FN(_cb)  # keep the trampoline alive
        check(lib().lio_engine_set_reduce_hook(self.h, self._hook, None))

    def set_joint(self, others=(), comm=None):
        """joint registration natively (lio_engine_set_joint): this engine drives the filter, `others` are engines holding further sub-maps on
        this GPU, `comm` (lio.Comm) joins the ranks that hold the rest"""
        self._joint_keep = (list(others), comm)
        hs = (C.c_void_p * max(len(others), 1))(*[o.h for o in others])
        check(lib().lio_engine_set_joint(self.h, hs, len(others), comm.h if comm is not None else None), "set_joint")

    def joint_register(self, raw, lidar_beg_time, state, cov):
        r = f32(raw).reshape(-1, 4)
        s, P = f64(state).copy(), f64(cov).reshape(-1).copy()
        rc = check(lib().lio_engine_joint_register(self.h, ptr(r, C.c_float), len(r), float(lidar_beg_time), ptr(s, C.c_double), ptr(P, C.c_double)),
                   "joint_register")
        return rc, s, P.reshape(23, 23)

    def joint_register_device(self, dptr, n, lidar_beg_time, state, cov):
        """lio_engine_joint_register_device: the cloud is already resident on the GPU"""
        s, P = f64(state).copy(), f64(cov).reshape(-1).copy()
        rc = check(lib().lio_engine_joint_register_device(self.h, C.c_void_p(dptr), n, float(lidar_beg_time), ptr(s, C.c_double), ptr(P, C.c_double)),
                   "joint_register_device")
        return rc, s, P.reshape(23, 23)

    def set_static_map(self, on=True):
        check(lib().lio_engine_set_static_map(self.h, int(on)))

    def flush(self):
        """lio_engine_flush: wait for the map_incremental the last scan enqueued; raises if the map overflowed"""
        check(lib().lio_engine_flush(self.h), "flush")

    def timings(self):
        t = capi.Timings()
        check(lib().lio_engine_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    @property
    def travel(self):
        return lib().lio_engine_travel(self.h)

    @property
    def is_degenerate(self):
        return bool(lib().lio_engine_is_degenerate(self.h))


def overlap_filter(cloud, xy_range=100.0, min_z=0.5):
    """`filter` of overlap_merge.hpp:213-223: keep sqrt(x^2 + y^2) < range && z > floor (f32)"""
    c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    d = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1])
    return c[(d < np.float32(xy_range)) & (c[:, 2] > np.float32(min_z))]


class Ndt:
    """The localization matcher (fast_gicp::NDTCuda, P2D): set_target = setInputTarget, the source is a Scan
    (upload + voxel_downsample = setInputSource), align = pcl::Registration::align(guess)."""

    def __init__(self, resolution=1.0, search_method=7, max_points=1_000_000, max_voxels=500_000, max_source_points=100_000, device=0):
        self.h = lib().lio_ndt_create(device, resolution, search_method, max_points, max_voxels, max_source_points)
        if not self.h:
            raise capi.LioError("lio_ndt_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_ndt_destroy(self.h)
        self.h = None

    __del__ = close

    def enable_kernel_timing(self, on=True):
        check(lib().lio_ndt_enable_kernel_timing(self.h, int(on)))

    def kernel_times(self, reset=True):
        t = capi.NdtTimes()
        check(lib().lio_ndt_kernel_times(self.h, C.byref(t), int(reset)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def set_target(self, pts):
        p = f32(pts).reshape(-1, 4)
        check(lib().lio_ndt_set_target(self.h, ptr(p, C.c_float), len(p)), "ndt set_target")

    def set_target_device(self, dptr, n):
        check(lib().lio_ndt_set_target_device(self.h, C.c_void_p(dptr), n), "ndt set_target (device)")

    @property
    def num_voxels(self):
        return check(lib().lio_ndt_num_voxels(self.h), "ndt num_voxels")

    def voxel_at(self, p):
        p = f32(p)
        mean, cinv = np.zeros(3, np.float32), np.zeros(9, np.float32)
        n = check(lib().lio_ndt_voxel_at(self.h, ptr(p, C.c_float), ptr(mean, C.c_float), ptr(cinv, C.c_float)), "ndt voxel_at")
        return n, mean, cinv.reshape(3, 3)

    def linearize(self, scan, T, update_corr=True, with_derivatives=True):
        T = f64(T).reshape(4, 4)
        H, b, e, nc = np.zeros(36), np.zeros(6), C.c_double(0), C.c_uint32(0)
        check(lib().lio_ndt_linearize(self.h, scan.h, ptr(T, C.c_double), int(update_corr), int(with_derivatives), ptr(H, C.c_double),
                                      ptr(b, C.c_double), C.byref(e), C.byref(nc)), "ndt linearize")
        return dict(n_corr=int(nc.value), H=H.reshape(6, 6), b=b, err=e.value)

    def fitness_score(self, scan, T, max_range=25.0):
        """pcl getFitnessScore(max_range): (mean squared nearest-neighbour distance, points within range)"""
        t = f64(T).reshape(4, 4)
        sc, ni = C.c_double(0.0), C.c_uint32(0)
        check(lib().lio_ndt_fitness_score(self.h, scan.h, ptr(t, C.c_double), float(max_range), C.byref(sc), C.byref(ni)), "fitness score")
        return sc.value, ni.value

    def overlap_score(self, scan, relpose, max_range=1.0, xy_range=100.0, min_z=0.5):
        """calc_fitness_score of overlap_merge.hpp:225-263 against this target (filter the target cloud with `overlap_filter` first):
        (mean squared nearest-neighbour distance of the inliers, inlier share of the filtered source)"""
        t = f64(relpose).reshape(4, 4)
        sc, ir = C.c_double(0.0), C.c_double(0.0)
        check(lib().lio_ndt_overlap_score(self.h, scan.h, ptr(t, C.c_double), float(max_range), float(xy_range), float(min_z), C.byref(sc), C.byref(ir)),
              "overlap score")
        return sc.value, ir.value

    def align(self, scan, guess, **params):
        g = f64(guess).reshape(4, 4)
        prm = capi.NdtParams()
        lib().lio_ndt_default_params(C.byref(prm))
        for k, v in params.items():
            setattr(prm, k, v)
        out = np.zeros((4, 4))
        it, conv = C.c_int(0), C.c_int(0)
        check(lib().lio_ndt_align(self.h, scan.h, ptr(g, C.c_double), C.byref(prm), ptr(out, C.c_double), C.byref(it), C.byref(conv)), "ndt align")
        return out, bool(conv.value), int(it.value)

    def prepare_batch(self, scans, guesses, targets=None):
        """the job array of lio_ndt_align_batch, marshalled once (so that a timed region can be the one C call); targets: one lio.Ndt per job
        (None = this one)"""
        n = len(scans)
        arr = (capi.AlignJob * n)()
        keep = [f64(g).reshape(16).copy() for g in guesses]
        for i in range(n):
            arr[i].target = targets[i].h if targets is not None and targets[i] is not None else None
            arr[i].source = scans[i].h
            arr[i].guess = ptr(keep[i], C.c_double)
        return arr, keep

    def run_batch(self, prepared, **params):
        arr, _ = prepared
        prm = capi.NdtParams()
        lib().lio_ndt_default_params(C.byref(prm))
        for k, v in params.items():
            setattr(prm, k, v)
        return lib().lio_ndt_align_batch(self.h, arr, len(arr), C.byref(prm))

    def align_batch(self, scans, guesses, targets=None, **params):
        """B alignments per launch against this target (lio_ndt_align_batch): scans = lio.Scan objects holding their downsampled clouds;
        returns a list of (T 4 x 4, converged, iterations, evaluations, rc)"""
        prep = self.prepare_batch(scans, guesses, targets)
        check(self.run_batch(prep, **params), "ndt align_batch")
        return [(np.array(a.out).reshape(4, 4), bool(a.converged), int(a.iterations), int(a.evaluations), int(a.rc)) for a in prep[0]]


class Gicp:
    """fast_gicp::FastGICP on the device (lio_gicp_*): 20-NN covariances with PLANE regularisation, nearest-neighbour correspondences,
    (C_B + R C_A R^T)^-1 cost, LM on SE(3)"""

    def __init__(self, grid_resolution=1.0, max_points=200_000, k=20, device=0):
        self.max_points = max_points
        self.h = lib().lio_gicp_create(device, float(grid_resolution), int(max_points), int(k))
        if not self.h:
            raise capi.LioError("lio_gicp_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_gicp_destroy(self.h)
        self.h = None

    __del__ = close

    def set_target(self, pts):
        p = f32(pts).reshape(-1, 4)
        check(lib().lio_gicp_set_target(self.h, ptr(p, C.c_float), len(p)), "gicp set_target")

    def set_source(self, pts):
        p = f32(pts).reshape(-1, 4)
        check(lib().lio_gicp_set_source(self.h, ptr(p, C.c_float), len(p)), "gicp set_source")

    def set_target_device(self, d_ptr, n):
        """a cloud that lies in HBM (d_ptr: device address of n float4) through set_target's path"""
        check(lib().lio_gicp_set_target_device(self.h, C.c_void_p(d_ptr), int(n)), "gicp set_target_device")

    def set_source_device(self, d_ptr, n):
        check(lib().lio_gicp_set_source_device(self.h, C.c_void_p(d_ptr), int(n)), "gicp set_source_device")

    def set_voxel_mode(self, voxel_resolution=1.0, search_method=1):
        """fast_gicp::FastVGICP: Gaussian-voxel target of `voxel_resolution` (0 = back to the kd-tree form), DIRECT1 / 7 / 27 lookup"""
        check(lib().lio_gicp_set_voxel_mode(self.h, float(voxel_resolution), int(search_method)), "gicp set_voxel_mode")

    def voxel_at(self, p):
        """(points in the target voxel holding p, mean (3,), covariance (3, 3)); 0 points = no such voxel"""
        p = f32(p)
        m, c = np.zeros(3), np.zeros(6)
        n = check(lib().lio_gicp_voxel_at(self.h, ptr(p, C.c_float), ptr(m, C.c_double), ptr(c, C.c_double)), "gicp voxel_at")
        return n, m, np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])

    def download(self, which):
        """(points (n, 4) in internal order, regularised covariances (n, 3, 3))"""
        pts, cov = np.zeros((self.max_points, 4), np.float32), np.zeros((self.max_points, 6))
        n = check(lib().lio_gicp_download(self.h, int(which), ptr(pts, C.c_float), ptr(cov, C.c_double), self.max_points), "gicp download")
        c = cov[:n]
        full = np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(n, 3, 3)
        return pts[:n].copy(), full

    def correspondences(self):
        out = np.zeros(self.max_points, np.int32)
        n = check(lib().lio_gicp_correspondences(self.h, ptr(out, C.c_int32), self.max_points), "gicp correspondences")
        return out[:n].copy()

    def neighbours(self, which):
        """(n, 32) int32: the sorted neighbour list of every point of cloud `which` in internal order (the point itself first or among its
        duplicates), -1 = an empty place; places >= k hold candidates no nearer than the k-th"""
        out = np.full((self.max_points, 32), -1, np.int32)
        n = check(lib().lio_gicp_neighbours(self.h, int(which), ptr(out, C.c_int32), self.max_points), "gicp neighbours")
        return out[:n].copy()

    def mahalanobis(self):
        """(n_source, 3, 3): (C_B + R C_A R^T)^-1 of the current pairs; rows without a pair are undefined"""
        m = np.zeros((self.max_points, 6))
        n = check(lib().lio_gicp_mahalanobis(self.h, ptr(m, C.c_double), self.max_points), "gicp mahalanobis")
        c = m[:n]
        return np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(n, 3, 3)

    def linearize(self, T, max_corr_dist=2.0, update_corr=True, with_derivatives=True):
        T = f64(T).reshape(4, 4)
        H, b, err, nc = np.zeros((6, 6)), np.zeros(6), C.c_double(0), C.c_uint32(0)
        check(lib().lio_gicp_linearize(self.h, ptr(T, C.c_double), float(max_corr_dist), int(update_corr), int(with_derivatives), ptr(H, C.c_double),
                                       ptr(b, C.c_double), C.byref(err), C.byref(nc)), "gicp linearize")
        return dict(H=H, b=b, err=err.value, n_corr=nc.value)

    def align(self, guess, max_corr_dist=2.0, **params):
        g = f64(guess).reshape(4, 4)
        prm = capi.NdtParams()
        lib().lio_ndt_default_params(C.byref(prm))
        prm.rotation_epsilon_deg, prm.transformation_epsilon, prm.max_iterations, prm.max_process_time_ms = 1e-2, 0.01, 64, -1.0
        for k, v in params.items():
            setattr(prm, k, v)
        out = np.zeros((4, 4))
        it, conv = C.c_int(0), C.c_int(0)
        check(lib().lio_gicp_align(self.h, ptr(g, C.c_double), C.byref(prm), float(max_corr_dist), ptr(out, C.c_double), C.byref(it), C.byref(conv)), "gicp align")
        return out, bool(conv.value), int(it.value)

    def fitness_score(self, T, max_range=25.0):
        """getFitnessScore(max_range) of the current pair under T -> (score, nr); max_range bounds the SQUARED distance"""
        T = f64(T).reshape(4, 4)
        sc, nr = C.c_double(0), C.c_uint32(0)
        check(lib().lio_gicp_fitness_score(self.h, ptr(T, C.c_double), float(max_range), C.byref(sc), C.byref(nr)), "gicp fitness_score")
        return sc.value, nr.value


class ScanContext:
    """SCManager of the relocalisation on the device (lio_sc_*): a bank of key-frame descriptors (20 rings x 60 sectors) resident in HBM,
    described many clouds at a time; the ring-key search, the column-shift distance and GlobalLocalization::globalSearch over it."""

    RINGS, SECTORS, CANDIDATES = 20, 60, 10
    SEARCH_SHIFTS = ((0, 0), (-4, 0), (4, 0), (0, -4), (0, 4), (-4, -4), (-4, 4), (4, -4), (4, 4))  # global_localization.cpp:388-390

    def __init__(self, max_frames=4096, max_points_per_call=1 << 20, device=0):
        self.h = lib().lio_sc_create(device, int(max_frames), int(max_points_per_call))
        if not self.h:
            raise capi.LioError("lio_sc_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_sc_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self):
        check(lib().lio_sc_reset(self.h), "sc reset")

    def num_frames(self):
        return check(lib().lio_sc_num_frames(self.h), "sc num_frames")

    def add_frames(self, clouds):
        """the clouds ((n_k, 4) f32 each) into the bank in one call; the id of the first"""
        clouds = [f32(c).reshape(-1, 4) for c in clouds]
        off = np.zeros(len(clouds) + 1, np.uint64)
        off[1:] = np.cumsum([len(c) for c in clouds])
        allp = np.ascontiguousarray(np.concatenate(clouds)) if clouds else np.zeros((0, 4), np.float32)
        return check(lib().lio_sc_add_frames_host(self.h, ptr(allp, C.c_float), ptr(off, C.c_uint64), len(clouds)), "sc add_frames")

    def download_frame(self, kid):
        """(descriptor (20, 60) f64, ring key (20,) f32, sector key (60,) f64)"""
        d, r, s = np.zeros((20, 60)), np.zeros(20, np.float32), np.zeros(60)
        check(lib().lio_sc_download_frame(self.h, int(kid), ptr(d, C.c_double), ptr(r, C.c_float), ptr(s, C.c_double)), "sc download_frame")
        return d, r, s

    def describe(self, cloud, shifts=((0.0, 0.0),)):
        """makeScancontext(cloud, dx, dy) per shift -> (descriptors (m, 20, 60), ring keys (m, 20) f32, sector keys (m, 60))"""
        p, sh = f32(cloud).reshape(-1, 4), f64(shifts).reshape(-1, 2)
        m = len(sh)
        d, r, s = np.zeros((m, 20, 60)), np.zeros((m, 20), np.float32), np.zeros((m, 60))
        check(lib().lio_sc_describe_host(self.h, ptr(p, C.c_float), len(p), ptr(sh, C.c_double), m, ptr(d, C.c_double), ptr(r, C.c_float), ptr(s, C.c_double)), "sc describe")
        return d, r, s

    def set_active(self, ids):
        """the frames a search looks at; None: every frame of the bank"""
        if ids is None:
            check(lib().lio_sc_set_active(self.h, None, -1), "sc set_active")
            return
        a = np.ascontiguousarray(ids, np.int32).ravel()
        check(lib().lio_sc_set_active(self.h, ptr(a, C.c_int32), len(a)), "sc set_active")

    def distance(self, desc_a, desc_b):
        """distanceBtnScanContext per pair -> (distances (n,), shifts (n,) int32)"""
        a, b = f64(desc_a).reshape(-1, 20, 60), f64(desc_b).reshape(-1, 20, 60)
        assert len(a) == len(b)
        n = len(a)
        d, s = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.int32)
        check(lib().lio_sc_distance(self.h, ptr(a, C.c_double), ptr(b, C.c_double), n, ptr(d, C.c_double), ptr(s, C.c_int32)), "sc distance")
        return d[:n], s[:n]

    def search(self, desc, ringkey):
        """per query the candidates in rising ring-key distance -> (ids (n, 10), distances (n, 10), shifts (n, 10), n_cand (n,))"""
        d, r = f64(desc).reshape(-1, 20, 60), f32(ringkey).reshape(-1, 20)
        assert len(d) == len(r)
        n = len(d)
        ids, dist, sh, nc = np.full((max(n, 1), 10), -1, np.int32), np.zeros((max(n, 1), 10)), np.zeros((max(n, 1), 10), np.int32), np.zeros(max(n, 1), np.int32)
        check(lib().lio_sc_search(self.h, ptr(d, C.c_double), ptr(r, C.c_float), n, ptr(ids, C.c_int32), ptr(dist, C.c_double), ptr(sh, C.c_int32), ptr(nc, C.c_int32)), "sc search")
        return ids[:n], dist[:n], sh[:n], nc[:n]

    def global_search(self, cloud, dist_thres=0.30):
        """globalSearch -> dict(match_id (-1: none), yaw (f32), score, shift)"""
        p = f32(cloud).reshape(-1, 4)
        mid, yaw, sc, sh = C.c_int32(0), C.c_float(0), C.c_double(0), C.c_int32(0)
        check(lib().lio_sc_global_search_host(self.h, ptr(p, C.c_float), len(p), float(dist_thres), C.byref(mid), C.byref(yaw), C.byref(sc), C.byref(sh)), "sc global_search")
        return dict(match_id=mid.value, yaw=np.float32(yaw.value), score=sc.value, shift=sh.value)

    def set_positions(self, xyz):
        """the key frames' positions ((F, 3), rounded to f32), row k = bank id k: what local_search measures the INS position against"""
        p = f32(xyz).reshape(-1, 3)
        check(lib().lio_sc_set_positions(self.h, ptr(p, C.c_float), len(p)), "sc set_positions")

    def local_search(self, cloud, ins_xyz, precision):
        """localSearch, the INS-aided start -> dict(match_id (-1: none), yaw (f32), score, shift, n_examined, ids, d2, dist, shifts): the last
        four are the min(10, F) frames nearest to (x, y, 0) in rising (d2, id) with the Scan Context distance and shift of each"""
        p, q = f32(cloud).reshape(-1, 4), f64(ins_xyz).reshape(3)
        mid, yaw, sc, ne, ms = C.c_int32(0), C.c_float(0), C.c_double(0), C.c_int32(0), C.c_int32(0)
        check(lib().lio_sc_local_search(self.h, ptr(p, C.c_float), len(p), ptr(q, C.c_double), float(precision), C.byref(mid), C.byref(yaw), C.byref(sc), C.byref(ne)),
              "sc local_search")
        ids, d2, dist, sh = np.zeros(10, np.int32), np.zeros(10, np.float32), np.zeros(10), np.zeros(10, np.int32)
        n = check(lib().lio_sc_last_local(self.h, ptr(ids, C.c_int32), ptr(d2, C.c_float), ptr(dist, C.c_double), ptr(sh, C.c_int32), C.byref(ms)), "sc last_local")
        return dict(match_id=mid.value, yaw=np.float32(yaw.value), score=sc.value, shift=ms.value, n_examined=ne.value, ids=ids[:n], d2=d2[:n], dist=dist[:n],
                    shifts=sh[:n])

    @staticmethod
    def shift_to_yaw(shift):
        return np.float32(lib().lio_sc_shift_to_yaw(int(shift)))

    def last_dropped(self):
        n = C.c_uint64(0)
        check(lib().lio_sc_last_dropped(self.h, C.byref(n)), "sc last_dropped")
        return n.value

    def last_times(self):
        v = [C.c_double(0) for _ in range(3)]
        check(lib().lio_sc_last_times(self.h, *[C.byref(x) for x in v]), "sc last_times")
        return dict(zip(("describe_us", "ringkey_us", "distance_us"), [x.value for x in v]))


class LoopDetector:
    """hdl_graph_slam::LoopDetector on the device (lio_loop_*): a bank of key frames with their covariances, find_candidates, all candidates
    aligned with FAST_VGICP in one batch (the LM loop on the device), nearest-neighbour fitness, FAST_GICP verification of the best.
    Keyword arguments override lio_loop_params."""

    REASONS = {0: "found", 1: "no_candidate", 2: "coarse_score", 3: "fine_not_converged", 4: "fine_score"}

    def __init__(self, device=0, **params):
        self.params = self.default_params()
        for k, v in params.items():
            if not hasattr(self.params, k):
                raise TypeError(f"lio_loop_params has no field {k!r}")
            setattr(self.params, k, v)
        self.h = lib().lio_loop_create(device, C.byref(self.params))
        if not self.h:
            raise capi.LioError("lio_loop_create failed: " + lib().lio_last_error().decode())

    @staticmethod
    def default_params():
        p = capi.LoopParams()
        lib().lio_loop_default_params(C.byref(p))
        return p

    @staticmethod
    def find_candidates(accum, pos_xy, new_accum, new_xy, last_edge_accum=0.0, params=None):
        """find_candidates (loop_detector.hpp:106-140) on the host: indices of the candidate key frames"""
        a, xy, nxy = f64(accum).ravel(), f64(pos_xy).reshape(-1, 2), f64(new_xy).ravel()
        out = np.zeros(max(len(a), 1), np.int32)
        n = check(lib().lio_loop_find_candidates(ptr(a, C.c_double), ptr(xy, C.c_double), len(a), float(new_accum), ptr(nxy, C.c_double), float(last_edge_accum),
                                                 C.byref(params) if params is not None else None, ptr(out, C.c_int32), len(out)), "loop find_candidates")
        return out[:n].copy()

    @staticmethod
    def information_matrix(fitness):
        out = np.zeros((6, 6))
        check(lib().lio_loop_information_matrix(float(fitness), ptr(out, C.c_double)), "loop information_matrix")
        return out

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_loop_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self):
        check(lib().lio_loop_reset(self.h), "loop reset")

    def add_keyframe(self, pts, pose, accum_distance):
        p, T = f32(pts).reshape(-1, 4), f64(pose).reshape(4, 4)
        return check(lib().lio_loop_add_keyframe_host(self.h, ptr(p, C.c_float), len(p), ptr(T, C.c_double), float(accum_distance)), "loop add_keyframe")

    def set_pose(self, kid, pose):
        T = f64(pose).reshape(4, 4)
        check(lib().lio_loop_set_pose(self.h, int(kid), ptr(T, C.c_double)), "loop set_pose")

    def retire(self, kid):
        """the frame leaves the matching for good (its id and storage stay): never again a new frame, a candidate or a neighbour"""
        check(lib().lio_loop_retire(self.h, int(kid)), "loop retire")

    def num_keyframes(self):
        q = C.c_int(0)
        n = check(lib().lio_loop_num_keyframes(self.h, C.byref(q)), "loop num_keyframes")
        return n, q.value

    def download_keyframe(self, kid):
        """(points (n, 4) in the bank's order, regularised covariances (n, 3, 3))"""
        n = -lib().lio_loop_download_keyframe(self.h, int(kid), None, None, 0)
        if n <= 0:
            raise capi.LioError(f"loop download_keyframe: no frame {kid}")
        pts, cov = np.zeros((n, 4), np.float32), np.zeros((n, 6))
        check(lib().lio_loop_download_keyframe(self.h, int(kid), ptr(pts, C.c_float), ptr(cov, C.c_double), n), "loop download_keyframe")
        full = np.stack([cov[:, 0], cov[:, 1], cov[:, 2], cov[:, 1], cov[:, 3], cov[:, 4], cov[:, 2], cov[:, 4], cov[:, 5]], 1).reshape(n, 3, 3)
        return pts, full

    @staticmethod
    def _edge(e):
        return dict(key1=int(e.key1), key2=int(e.key2), relative_pose=np.array(e.relative_pose, np.float32).reshape(4, 4), score=float(e.score),
                    information=np.array(e.information).reshape(6, 6))

    def detect(self, cap=16):
        """detect() over the queued key frames -> the loops of this call, each a dict key1, key2, relative_pose, score, information"""
        buf = (capi.LoopEdge * cap)()
        n = lib().lio_loop_detect(self.h, buf, cap)
        if n < -cap:  # more loops than cap: they are the tail of edges()
            return self.edges()[n:]
        check(n, "loop detect")
        return [self._edge(buf[i]) for i in range(n)]

    def edges(self):
        n = lib().lio_loop_edges(self.h, None, 0)
        n = -n if n < 0 else n
        if n == 0:
            return []
        buf = (capi.LoopEdge * n)()
        check(lib().lio_loop_edges(self.h, buf, n), "loop edges")
        return [self._edge(buf[i]) for i in range(n)]

    def last_report(self):
        rep = capi.LoopReport()
        K = abs(lib().lio_loop_last_report(self.h, C.byref(rep), None, None, None, None, 0))
        ids, conv, it, sc = np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1))
        check(lib().lio_loop_last_report(self.h, C.byref(rep), ptr(ids, C.c_int32), ptr(conv, C.c_int32), ptr(it, C.c_int32), ptr(sc, C.c_double), max(K, 1)), "loop last_report")
        return dict(new_id=rep.new_id, candidates=ids[:K].copy(), converged=conv[:K].astype(bool), iterations=it[:K].copy(), scores=sc[:K].copy(), best=rep.best,
                    best_score=rep.best_score, fine_converged=bool(rep.fine_converged), fine_iterations=rep.fine_iterations, fine_score=rep.fine_score,
                    reason=self.REASONS.get(rep.reason, str(rep.reason)), coarse_rounds=rep.coarse_rounds)

    def last_times(self):
        v = [C.c_double(0) for _ in range(5)]
        check(lib().lio_loop_last_times(self.h, *[C.byref(x) for x in v]), "loop last_times")
        return dict(zip(("insert_us", "target_us", "coarse_us", "fitness_us", "fine_us"), [x.value for x in v]))

    def align_candidates(self, target_id, source_ids, guesses):
        """the coarse batch + fitness: per job (T (4, 4) f64, converged, iterations, score, nr)"""
        ids = np.ascontiguousarray(source_ids, np.int32).ravel()
        g = f64(guesses).reshape(-1, 4, 4)
        n = len(ids)
        assert len(g) == n
        T, it, conv, sc, nr = np.zeros((max(n, 1), 4, 4)), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1)), np.zeros(max(n, 1), np.uint32)
        check(lib().lio_loop_align_candidates(self.h, int(target_id), ptr(ids, C.c_int32), n, ptr(g, C.c_double), ptr(T, C.c_double), ptr(it, C.c_int32),
                                              ptr(conv, C.c_int32), ptr(sc, C.c_double), ptr(nr, C.c_uint32)), "loop align_candidates")
        return [(T[i].copy(), bool(conv[i]), int(it[i]), float(sc[i]), int(nr[i])) for i in range(n)]

    def align_fine(self, target_id, source_id, guess):
        g, T = f64(guess).reshape(4, 4), np.zeros((4, 4))
        it, conv, sc, nr = C.c_int32(0), C.c_int32(0), C.c_double(0), C.c_uint32(0)
        check(lib().lio_loop_align_fine(self.h, int(target_id), int(source_id), ptr(g, C.c_double), ptr(T, C.c_double), C.byref(it), C.byref(conv), C.byref(sc), C.byref(nr)),
              "loop align_fine")
        return T, bool(conv.value), int(it.value), sc.value, nr.value

    def pair_information(self, id1, id2, relpose):
        """calc_information_matrix(cloud1, cloud2, relpose): frame id2 moved by relpose (cast to f32) against frame id1's exact nearest
        neighbours, every point counting -> (score, nr, information (6, 6))"""
        T, info = f64(relpose).reshape(4, 4), np.zeros((6, 6))
        sc, nr = C.c_double(0), C.c_uint32(0)
        check(lib().lio_loop_pair_information(self.h, int(id1), int(id2), ptr(T, C.c_double), C.byref(sc), C.byref(nr), ptr(info, C.c_double)), "loop pair_information")
        return sc.value, nr.value, info


class OverlapDetector:
    """OverlapDetector of the reference's map merge on the device (lio_overlap_*) over a LoopDetector's bank: the key frames of both maps are
    added to `bank` and addressed by bank id.  find_candidates and connection_count run on the host; gate, align_pairs and accumulate are the
    stage doors; detect is one detect() call over a fragment of new frames.  Keyword arguments override lio_overlap_params.  The bank must
    outlive the detector."""

    REASONS = {0: "found", 1: "no_candidate", 2: "gate", 3: "coarse", 4: "fine_not_converged", 5: "fine_score"}
    ACCUM = capi.OVERLAP_ACCUM

    def __init__(self, bank, **params):
        self.bank = bank
        self.params = self.default_params(bank)
        for k, v in params.items():
            if not hasattr(self.params, k):
                raise TypeError(f"lio_overlap_params has no field {k!r}")
            setattr(self.params, k, v)
        self.h = lib().lio_overlap_create(bank.h, C.byref(self.params))
        if not self.h:
            raise capi.LioError("lio_overlap_create failed: " + lib().lio_last_error().decode())

    @staticmethod
    def default_params(bank=None):
        p = capi.OverlapParams()
        lib().lio_overlap_default_params(bank.h if bank is not None else None, C.byref(p))
        return p

    @staticmethod
    def _edges(edges):
        e = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        return np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])

    @staticmethod
    def connection_count(edges, source, target, max_count):
        """get_connection_count (overlap_merge.hpp:265-296) over the undirected edges (m, 2): breadth-first LEVELS from source until target"""
        a, b = OverlapDetector._edges(edges)
        return check(lib().lio_overlap_connection_count(ptr(a, C.c_int32), ptr(b, C.c_int32), len(a), int(source), int(target), int(max_count)), "overlap connection_count")

    @staticmethod
    def find_candidates(pos_xyz, ids, edges, new_id, new_xyz, params=None):
        """find_candidates (overlap_merge.hpp:113-145) on the host: indices into the key frames, in the order they were accepted"""
        pos, kid, q = f64(pos_xyz).reshape(-1, 3), np.ascontiguousarray(ids, np.int32).ravel(), f64(new_xyz).ravel()
        assert len(pos) == len(kid) and len(q) == 3
        a, b = OverlapDetector._edges(edges)
        out = np.zeros(max(len(kid), 1), np.int32)
        n = check(lib().lio_overlap_find_candidates(ptr(pos, C.c_double), ptr(kid, C.c_int32), len(kid), ptr(a, C.c_int32), ptr(b, C.c_int32), len(a), int(new_id),
                                                    ptr(q, C.c_double), C.byref(params) if params is not None else None, ptr(out, C.c_int32), len(out)),
                  "overlap find_candidates")
        return out[:n].copy()

    def close(self):
        if getattr(self, "h", None) and lib is not None and getattr(self.bank, "h", None):
            lib().lio_overlap_destroy(self.h)
        self.h = None

    __del__ = close

    def gate(self, target_id, source_ids, Ts, max_range=1.0):
        """calc_fitness_score (overlap_merge.hpp:225-263) of bank frames source_ids moved by Ts against bank frame target_id (ACCUM: the
        accumulated cloud): per pair (score, nr, n_in); the inlier ratio is nr / n_in"""
        ids, T = np.ascontiguousarray(source_ids, np.int32).ravel(), f64(Ts).reshape(-1, 4, 4)
        n = len(ids)
        assert len(T) == n
        sc, nr, nin = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        check(lib().lio_overlap_gate_batch(self.h, int(target_id), ptr(ids, C.c_int32), n, ptr(T, C.c_double), float(max_range), ptr(sc, C.c_double),
                                           ptr(nr, C.c_uint32), ptr(nin, C.c_uint32)), "overlap gate")
        return [(float(sc[i]), int(nr[i]), int(nin[i])) for i in range(n)]

    def align_pairs(self, target_ids, source_ids, guesses):
        """FAST_VGICP of (target, source) pairs of bank frames in one set of rounds: per pair (T (4, 4) f64, converged, iterations)"""
        t, s = np.ascontiguousarray(target_ids, np.int32).ravel(), np.ascontiguousarray(source_ids, np.int32).ravel()
        g = f64(guesses).reshape(-1, 4, 4)
        n = len(t)
        assert len(s) == n and len(g) == n
        T, it, conv = np.zeros((max(n, 1), 4, 4)), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        check(lib().lio_overlap_align_pairs(self.h, ptr(t, C.c_int32), ptr(s, C.c_int32), n, ptr(g, C.c_double), ptr(T, C.c_double), ptr(it, C.c_int32),
                                            ptr(conv, C.c_int32)), "overlap align_pairs")
        return [(T[i].copy(), bool(conv[i]), int(it[i])) for i in range(n)]

    def accumulate(self, best_id, neighbour_ids):
        """the fine target: best's cloud, then every neighbour's moved by best.pose^-1 * neighbour.pose -> (points (n, 4), covariances (n, 3, 3))"""
        nb = np.ascontiguousarray(neighbour_ids, np.int32).ravel()
        n = check(lib().lio_overlap_accumulate(self.h, int(best_id), ptr(nb, C.c_int32), len(nb)), "overlap accumulate")
        pts, cov = np.zeros((n, 4), np.float32), np.zeros((n, 6))
        check(lib().lio_overlap_download_accum(self.h, ptr(pts, C.c_float), ptr(cov, C.c_double), n), "overlap download_accum")
        full = np.stack([cov[:, 0], cov[:, 1], cov[:, 2], cov[:, 1], cov[:, 3], cov[:, 4], cov[:, 2], cov[:, 4], cov[:, 5]], 1).reshape(n, 3, 3)
        return pts, full

    def detect(self, ref_ids, new_ids, edges, ref_kf=None, new_kf=None, cap=64):
        """one detect() call: bank ids of the reference map's frames and of the fragment, the graph's edges (m, 2) in key-frame ids (ref_kf /
        new_kf: the frames' key-frame ids, default the bank ids) -> the overlaps, each a dict key1 (best), key2 (new), relative_pose, score,
        information"""
        r, w = np.ascontiguousarray(ref_ids, np.int32).ravel(), np.ascontiguousarray(new_ids, np.int32).ravel()
        rk = np.ascontiguousarray(ref_kf, np.int32).ravel() if ref_kf is not None else None
        wk = np.ascontiguousarray(new_kf, np.int32).ravel() if new_kf is not None else None
        assert (rk is None or len(rk) == len(r)) and (wk is None or len(wk) == len(w))
        a, b = self._edges(edges)
        cap = max(cap, len(w), 1)
        buf = (capi.OverlapEdge * cap)()
        n = check(lib().lio_overlap_detect(self.h, ptr(r, C.c_int32), ptr(rk, C.c_int32) if rk is not None else None, len(r), ptr(w, C.c_int32),
                                           ptr(wk, C.c_int32) if wk is not None else None, len(w), ptr(a, C.c_int32), ptr(b, C.c_int32), len(a), buf, cap), "overlap detect")
        self._n_new = len(w)
        return [LoopDetector._edge(buf[i]) for i in range(n)]

    def last_report(self, k=None):
        """the report of new frame k of the last detect (None: a list over all its frames)"""
        if k is None:
            return [self.last_report(i) for i in range(getattr(self, "_n_new", 0))]
        rep = capi.OverlapReport()
        K = abs(lib().lio_overlap_last_report(self.h, int(k), C.byref(rep), None, None, None, None, None, 0))  # -(count): the arrays were too small
        m = max(K, 1)
        ids, ratio, conv, it, sc = np.zeros(m, np.int32), np.zeros(m), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m)
        check(lib().lio_overlap_last_report(self.h, int(k), C.byref(rep), ptr(ids, C.c_int32), ptr(ratio, C.c_double), ptr(conv, C.c_int32), ptr(it, C.c_int32),
                                            ptr(sc, C.c_double), m), "overlap last_report")
        return dict(new_id=rep.new_id, candidates=ids[:K].copy(), gate_ratio=ratio[:K].copy(), converged=conv[:K].astype(bool), iterations=it[:K].copy(),
                    scores=sc[:K].copy(), best=rep.best, best_score=rep.best_score, fine_converged=bool(rep.fine_converged), fine_iterations=rep.fine_iterations,
                    fine_score=rep.fine_score, n_accum=rep.n_accum, n_neighbours_skipped=rep.n_neighbours_skipped, n_neighbours_dropped=rep.n_neighbours_dropped, reason=self.REASONS.get(rep.reason, str(rep.reason)))

    def last_times(self):
        t = capi.OverlapTimes()
        check(lib().lio_overlap_last_times(self.h, C.byref(t)), "overlap last_times")
        return {k: getattr(t, k) for k, _ in capi.OverlapTimes._fields_ if k != "pad"}


class PoseGraph:
    """The pose graph on the device (lio_graph_*): SE3 nodes, EdgeSE3 edges with an optional Huber kernel, Levenberg-Marquardt as g2o's
    OptimizationAlgorithmLevenberg runs it, the linear solve by block-Jacobi conjugate gradients.  Keyword arguments override lio_graph_params."""

    NONE, HUBER = capi.GRAPH_KERNEL_NONE, capi.GRAPH_KERNEL_HUBER
    DCS2 = capi.GRAPH_KERNEL_DCS2
    XYZ, QUAT, PLANE = capi.GRAPH_PRIOR_XYZ, capi.GRAPH_PRIOR_QUAT, capi.GRAPH_PRIOR_PLANE
    STOPS = {0: "none", 1: "max_iterations", 2: "trials", 3: "rho_zero", 4: "lambda", 5: "chi2_rel"}

    def __init__(self, device=0, **params):
        self.params = self.default_params()
        for k, v in params.items():
            if not hasattr(self.params, k):
                raise TypeError(f"lio_graph_params has no field {k!r}")
            setattr(self.params, k, v)
        self.h = lib().lio_graph_create(device, C.byref(self.params))
        if not self.h:
            raise capi.LioError("lio_graph_create failed: " + lib().lio_last_error().decode())

    @staticmethod
    def default_params():
        p = capi.GraphParams()
        lib().lio_graph_default_params(C.byref(p))
        return p

    @staticmethod
    def from_mqt(v6):
        v, T = f64(v6).ravel(), np.zeros((4, 4))
        lib().lio_se3_from_mqt(ptr(v, C.c_double), ptr(T, C.c_double))
        return T

    @staticmethod
    def to_mqt(T):
        M, v = f64(T).reshape(4, 4), np.zeros(6)
        lib().lio_se3_to_mqt(ptr(M, C.c_double), ptr(v, C.c_double))
        return v

    @staticmethod
    def edge_error(x_from, x_to, m):
        a, b, c, e = f64(x_from).reshape(4, 4), f64(x_to).reshape(4, 4), f64(m).reshape(4, 4), np.zeros(6)
        check(lib().lio_graph_edge_error(ptr(a, C.c_double), ptr(b, C.c_double), ptr(c, C.c_double), ptr(e, C.c_double)), "graph edge_error")
        return e

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_graph_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self):
        check(lib().lio_graph_reset(self.h), "graph reset")

    def add_node(self, pose, fixed=False):
        T = f64(pose).reshape(4, 4)
        nid = check(lib().lio_graph_add_node(self.h, ptr(T, C.c_double)), "graph add_node")
        if fixed:
            self.set_fixed(nid, True)
        return nid

    def set_fixed(self, nid, flag=True):
        check(lib().lio_graph_set_fixed(self.h, int(nid), int(bool(flag))), "graph set_fixed")

    def set_estimate(self, nid, pose):
        T = f64(pose).reshape(4, 4)
        check(lib().lio_graph_set_estimate(self.h, int(nid), ptr(T, C.c_double)), "graph set_estimate")

    def add_edge(self, i, j, measurement, information, kernel=0, delta=1.0):
        M, W = f64(measurement).reshape(4, 4), f64(information).reshape(6, 6)
        return check(lib().lio_graph_add_edge(self.h, int(i), int(j), ptr(M, C.c_double), ptr(W, C.c_double), int(kernel), float(delta)), "graph add_edge")

    def remove_edge(self, eid):
        check(lib().lio_graph_remove_edge(self.h, int(eid)), "graph remove_edge")

    def remove_node(self, nid):
        """the node and every edge and prior on it leave the graph; ids stay, the removed id is unknown from here on"""
        check(lib().lio_graph_remove_node(self.h, int(nid)), "graph remove_node")

    def node_live(self):
        n = self.num_nodes
        out = np.zeros(max(n, 1), np.uint8)
        check(lib().lio_graph_node_live(self.h, ptr(out, C.c_uint8), len(out)), "graph node_live")
        return out[:n].astype(bool)

    def edge_records(self):
        """the live binary edges in rising id as they were added: a list of dicts (id, from, to, measurement (4, 4), information (6, 6), kernel, delta)"""
        n = abs(lib().lio_graph_edge_records(self.h, None, None, None, None, None, None, None, 0))
        c = max(n, 1)
        i, a, b, kn = (np.zeros(c, np.int32) for _ in range(4))
        M, W, dl = np.zeros((c, 4, 4)), np.zeros((c, 6, 6)), np.zeros(c)
        check(lib().lio_graph_edge_records(self.h, ptr(i, C.c_int32), ptr(a, C.c_int32), ptr(b, C.c_int32), ptr(M, C.c_double), ptr(W, C.c_double), ptr(kn, C.c_int32),
                                           ptr(dl, C.c_double), c), "graph edge_records")
        return [{"id": int(i[k]), "from": int(a[k]), "to": int(b[k]), "measurement": M[k].copy(), "information": W[k].copy(), "kernel": int(kn[k]),
                 "delta": float(dl[k])} for k in range(n)]

    @staticmethod
    def _prior_args(kind, measurement, plane):
        m = np.zeros(4)
        v = f64(measurement).ravel()
        m[:len(v)] = v
        pl = f64(plane).ravel() if plane is not None else None
        return m, pl, (ptr(pl, C.c_double) if pl is not None else None)

    @staticmethod
    def prior_error(pose, kind, measurement, plane=None):
        X, e = f64(pose).reshape(4, 4), np.zeros(3)
        m, pl, plp = PoseGraph._prior_args(kind, measurement, plane)
        check(lib().lio_graph_prior_error(ptr(X, C.c_double), int(kind), ptr(m, C.c_double), plp, ptr(e, C.c_double)), "graph prior_error")
        return e

    def add_prior(self, node, kind, measurement, information, kernel=0, delta=1.0, plane=None):
        """a unary edge on one node: XYZ (x, y, z), QUAT (x, y, z, w) or PLANE (n, d in the node's frame, with the world plane); -> its edge id"""
        m, pl, plp = self._prior_args(kind, measurement, plane)
        W = f64(information).reshape(3, 3)
        return check(lib().lio_graph_add_prior(self.h, int(node), int(kind), ptr(m, C.c_double), plp, ptr(W, C.c_double), int(kernel), float(delta)), "graph add_prior")

    def set_kernel(self, eid, kernel, delta=1.0):
        check(lib().lio_graph_set_kernel(self.h, int(eid), int(kernel), float(delta)), "graph set_kernel")

    def priors(self):
        """the live priors in rising id: a list of dicts (id, node, type, measurement (4,), plane (4,), information (3, 3), kernel, delta)"""
        n = abs(lib().lio_graph_priors(self.h, None, None, None, None, None, None, None, None, 0))
        c = max(n, 1)
        i, nd, ty, kn = (np.zeros(c, np.int32) for _ in range(4))
        m, pl, W, dl = np.zeros((c, 4)), np.zeros((c, 4)), np.zeros((c, 3, 3)), np.zeros(c)
        check(lib().lio_graph_priors(self.h, ptr(i, C.c_int32), ptr(nd, C.c_int32), ptr(ty, C.c_int32), ptr(m, C.c_double), ptr(pl, C.c_double), ptr(W, C.c_double),
                                     ptr(kn, C.c_int32), ptr(dl, C.c_double), c), "graph priors")
        return [dict(id=int(i[k]), node=int(nd[k]), type=int(ty[k]), measurement=m[k].copy(), plane=pl[k].copy(), information=W[k].copy(), kernel=int(kn[k]),
                     delta=float(dl[k])) for k in range(n)]

    def remove_gnss_outliers(self, max_distance_error=1.0, max_iterations=1024):
        """the GNSS outlier stage -> (ids removed, or None when the graph has fewer than min_edges live edges; the second optimisation's report)"""
        cap = max(len(self.edges()[0]), 1)
        ids, rep = np.zeros(cap, np.int32), capi.GraphReport()
        below = len(self.edges()[0]) < self.params.min_edges
        n = lib().lio_graph_remove_gnss_outliers(self.h, float(max_distance_error), int(max_iterations), ptr(ids, C.c_int32), cap, C.byref(rep))
        if n == -1 and below:
            return None, {}
        check(n, "graph remove_gnss_outliers")
        d = {k: getattr(rep, k) for k, _ in capi.GraphReport._fields_}
        d["lambda"] = d.pop("lambda_")
        d["stop"] = self.STOPS.get(rep.stop_reason, str(rep.stop_reason))
        return [int(x) for x in ids[:n]], d

    def _report(self, rep):
        d = {k: getattr(rep, k) for k, _ in capi.GraphReport._fields_}
        d["lambda"] = d.pop("lambda_")
        d["stop"] = self.STOPS.get(rep.stop_reason, str(rep.stop_reason))
        return d

    def estimate_gnss_moment(self, max_distance_error=1.0, max_iterations=1024, prior_information=None):
        """the GNSS moment stage -> (the number of XYZ priors re-anchored, the moment (3,), the stage's report); (0, zeros, {}) with nothing
        touched when there is no live XYZ prior.  With fixes z = t + R l the moment comes out near -l"""
        W = f64(prior_information).reshape(3, 3) if prior_information is not None else None
        m, rep = np.zeros(3), capi.GraphReport()
        n = check(lib().lio_graph_estimate_gnss_moment(self.h, float(max_distance_error), int(max_iterations), ptr(W, C.c_double) if W is not None else None,
                                                       ptr(m, C.c_double), C.byref(rep)), "graph estimate_gnss_moment")
        return n, m, (self._report(rep) if n else {})

    def moment_begin(self, m0=None, prior_information=None):
        """opens the moment stage: until moment_end, optimize / chi2 / linearize run over the bordered system"""
        m = f64(m0).ravel() if m0 is not None else None
        W = f64(prior_information).reshape(3, 3) if prior_information is not None else None
        check(lib().lio_graph_moment_begin(self.h, ptr(m, C.c_double) if m is not None else None, ptr(W, C.c_double) if W is not None else None), "graph moment_begin")

    def moment_end(self, apply=True):
        """closes the stage; apply: every live XYZ prior's measurement moves to z + R m -> their number"""
        return check(lib().lio_graph_moment_end(self.h, int(bool(apply))), "graph moment_end")

    def moment(self):
        m = np.zeros(3)
        check(lib().lio_graph_moment_get(self.h, ptr(m, C.c_double)), "graph moment")
        return m

    def linearize_moment(self):
        """one linearisation of the open stage -> b_m (3,), H_mm (3, 3), H_pm (N, 6, 3): zeros for a node that is fixed or has no moment edge"""
        N = self.num_nodes
        bm, Hmm, Hpm = np.zeros(3), np.zeros((3, 3)), np.zeros((max(N, 1), 6, 3))
        check(lib().lio_graph_moment_linearize(self.h, ptr(bm, C.c_double), ptr(Hmm, C.c_double), ptr(Hpm, C.c_double), len(Hpm)), "graph moment_linearize")
        return bm, Hmm, Hpm[:N]

    @property
    def num_nodes(self):
        return check(lib().lio_graph_num_nodes(self.h), "graph num_nodes")

    def fixed(self):
        n = self.num_nodes
        out = np.zeros(max(n, 1), np.uint8)
        check(lib().lio_graph_get_fixed(self.h, ptr(out, C.c_uint8), len(out)), "graph get_fixed")
        return out[:n].astype(bool)

    def optimize(self, max_iterations=1024):
        """-> (iterations run, or -1 when the graph has fewer than min_edges live edges and nothing was touched; the report as a dict)"""
        rep = capi.GraphReport()
        n = lib().lio_graph_optimize(self.h, int(max_iterations), C.byref(rep))
        if n < -1 or (n == -1 and len(self.edges()[0]) >= self.params.min_edges):
            check(n, "graph optimize")
        d = {k: getattr(rep, k) for k, _ in capi.GraphReport._fields_}
        d["lambda"] = d.pop("lambda_")
        d["stop"] = self.STOPS.get(rep.stop_reason, str(rep.stop_reason))
        return n, d

    def estimates(self):
        n = self.num_nodes
        out = np.zeros((max(n, 1), 4, 4))
        check(lib().lio_graph_estimates(self.h, ptr(out, C.c_double), len(out)), "graph estimates")
        return out[:n]

    def edges(self):
        """the live edges: (from, to, id)"""
        n = abs(lib().lio_graph_edges(self.h, None, None, None, 0))
        a, b, c = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        check(lib().lio_graph_edges(self.h, ptr(a, C.c_int32), ptr(b, C.c_int32), ptr(c, C.c_int32), max(n, 1)), "graph edges")
        return a[:n], b[:n], c[:n]

    def chi2(self):
        v = C.c_double(0)
        check(lib().lio_graph_chi2(self.h, C.byref(v)), "graph chi2")
        return v.value

    def linearize(self, n_edge_ids):
        """one linearisation at the current estimate: errors (E, 6), chi2 (E,), rho' (E,), b (N, 6), the diagonal blocks (N, 6, 6)"""
        E, N = int(n_edge_ids), self.num_nodes
        err, c2, r1, b, Hd = np.zeros((max(E, 1), 6)), np.zeros(max(E, 1)), np.zeros(max(E, 1)), np.zeros((max(N, 1), 6)), np.zeros((max(N, 1), 6, 6))
        got = check(lib().lio_graph_linearize(self.h, ptr(err, C.c_double), ptr(c2, C.c_double), ptr(r1, C.c_double), len(c2), ptr(b, C.c_double), ptr(Hd, C.c_double),
                                              len(b)), "graph linearize")
        assert got == E, (got, E)
        return err[:E], c2[:E], r1[:E], b[:N], Hd[:N]

    def last_times(self):
        v = [C.c_double(0) for _ in range(4)]
        check(lib().lio_graph_last_times(self.h, *[C.byref(x) for x in v]), "graph last_times")
        return dict(zip(("linearize_us", "assemble_us", "solve_us", "update_us"), [x.value for x in v]))


class Cloud:
    """lio_cloud: a device-resident cloud that grows over a drive, and pcl::VoxelGrid over all of it (the dense-map export of
    graph_utils.cpp:160-200, 410-446).  Appends transform (f64, as pcl::transformPointCloud with a Matrix4d), scale the intensity, keep an
    inclusive z band and keep the input order."""

    def __init__(self, reserve=0, device=0):
        self.h = lib().lio_cloud_create(device, int(reserve))
        if not self.h:
            raise capi.LioError("lio_cloud_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_cloud_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def _args(T, intensity_scale, z_band):
        M = np.eye(4) if T is None else np.ascontiguousarray(T, np.float64).reshape(4, 4)
        M = np.ascontiguousarray(M, np.float64)
        band = z_band is not None
        lo, hi = (float(z_band[0]), float(z_band[1])) if band else (0.0, 0.0)
        return M, float(intensity_scale), int(band), lo, hi

    def append_host(self, xyzi, T=None, intensity_scale=1.0, z_band=None):
        p = f32(xyzi).reshape(-1, 4)
        M, sc, band, lo, hi = self._args(T, intensity_scale, z_band)
        check(lib().lio_cloud_append_host(self.h, ptr(p, C.c_float), len(p), ptr(M, C.c_double), sc, band, lo, hi), "cloud append_host")

    def append_scan(self, scan, T=None, intensity_scale=1.0, z_band=None):
        M, sc, band, lo, hi = self._args(T, intensity_scale, z_band)
        check(lib().lio_cloud_append_scan(self.h, scan.h, ptr(M, C.c_double), sc, band, lo, hi), "cloud append_scan")

    def clear(self):
        check(lib().lio_cloud_clear(self.h), "cloud clear")

    @property
    def size(self):
        n = C.c_uint64(0)
        check(lib().lio_cloud_size(self.h, C.byref(n)), "cloud size")
        return int(n.value)

    def voxel_downsample(self, leaf):
        n = C.c_uint64(0)
        check(lib().lio_cloud_voxel_downsample(self.h, float(leaf), C.byref(n)), "cloud voxel downsample")
        return int(n.value)

    def download(self):
        n = self.size
        out = np.zeros((n, 4), np.float32)
        m = lib().lio_cloud_download(self.h, ptr(out, C.c_float), n)
        check(m if m >= 0 else capi.LIO_E_CAPACITY, "cloud download")
        return out[:m]

    def scratch_bytes(self):
        b = C.c_uint64(0)
        check(lib().lio_cloud_scratch_bytes(self.h, C.byref(b)), "cloud scratch bytes")
        return int(b.value)

    def last_times(self):
        """(append_us, voxel_us): device time of the last append and of the last voxel grid"""
        a, v = C.c_double(0), C.c_double(0)
        check(lib().lio_cloud_last_times(self.h, C.byref(a), C.byref(v)), "cloud times")
        return a.value, v.value


class KnnIndex:
    """lio_knn_index: exact k nearest neighbours over a static cloud (pcl::KdTreeFLANN<PointXYZRGB> of texture_mesh, graph_utils.cpp:449-501).
    Only finite points are indexed; distances are ((dx*dx) + dy*dy) + dz*dz in f32; results ascend in (d2, index), ties going to the smaller
    input index; missing slots are (-1, +inf); a non-finite query has no neighbours."""

    def __init__(self, device=0):
        self.h = lib().lio_knn_index_create(device)
        if not self.h:
            raise capi.LioError("lio_knn_index_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_knn_index_destroy(self.h)
        self.h = None

    __del__ = close

    def build(self, xyz, rgb=None):
        """xyz: n x 3; rgb: n packed 0x??RRGGBB words or None.  Returns the number of points indexed (the finite ones)."""
        p = f32(xyz).reshape(-1, 3)
        c = None if rgb is None else np.ascontiguousarray(rgb, np.uint32).reshape(-1)
        if c is not None and len(c) != len(p):
            raise ValueError("KnnIndex.build: one colour per point")
        nf = C.c_uint64(0)
        check(lib().lio_knn_index_build(self.h, ptr(p, C.c_float), None if c is None else ptr(c, C.c_uint32), len(p), C.byref(nf)), "knn index build")
        return int(nf.value)

    def query(self, q, k):
        """(idx int32 m x k, d2 f32 m x k)"""
        p = f32(q).reshape(-1, 3)
        idx = np.empty((len(p), k), np.int32)
        d2 = np.empty((len(p), k), np.float32)
        check(lib().lio_knn_index_query(self.h, ptr(p, C.c_float), len(p), int(k), ptr(idx, C.c_int32), ptr(d2, C.c_float)), "knn index query")
        return idx, d2

    def colour(self, q, k=3):
        """m x 3 uint8: floor-mean of the r, g, b bytes of each query's (up to) k neighbours; none -> 0, 0, 0"""
        p = f32(q).reshape(-1, 3)
        out = np.empty((len(p), 3), np.uint8)
        check(lib().lio_knn_index_colour(self.h, ptr(p, C.c_float), len(p), int(k), ptr(out, C.c_uint8)), "knn index colour")
        return out

    def last_times(self):
        """(build_us, query_us): device time of the last build and of the last query / colour call"""
        b, q = C.c_double(0), C.c_double(0)
        check(lib().lio_knn_index_last_times(self.h, C.byref(b), C.byref(q)), "knn index times")
        return b.value, q.value


class GroundDetector:
    """lio_ground: detect_ground of graph_utils.cpp:329-382 (the floor detector of floor_detection_nodelet.cpp:79-193) on the device: height
    clip, normals from the 10 nearest neighbours, verticality filter, plane RANSAC, inlier cloud.  The draws of the RANSAC are this project's
    (a counter-based generator of (seed, draw number), include/lio_hip.h; `ground_draw` restates it), not PCL's: the same seed gives the same
    result on every run."""

    def __init__(self, device=0):
        self.h = lib().lio_ground_create(device)
        if not self.h:
            raise capi.LioError("lio_ground_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_ground_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def params(preset=0, **over):
        """lio_ground_params of a preset (0: detect_ground, clip 1.5 / 1.5; 1: the floor detector, clip 2.0 / 1.0), fields overridden by name"""
        p = capi.GroundParams()
        lib().lio_ground_default_params(C.byref(p), int(preset))
        for k, v in over.items():
            if not hasattr(p, k):
                raise ValueError(f"lio_ground_params has no field {k}")
            setattr(p, k, v)
        return p

    def _result(self, found, co, nc, nf, ni):
        return dict(found=bool(found.value), coeffs=co.copy() if found.value else None, n_clipped=int(nc.value), n_filtered=int(nf.value),
                    n_inliers=int(ni.value))

    def detect_scan(self, scan, params=None, replace=False):
        p = params if params is not None else self.params()
        found, co = C.c_int(0), np.zeros(4, np.float32)
        nc, nf, ni = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().lio_ground_detect_scan(self.h, scan.h, C.byref(p), int(bool(replace)), C.byref(found), ptr(co, C.c_float), C.byref(nc), C.byref(nf),
                                           C.byref(ni)), "ground detect_scan")
        return self._result(found, co, nc, nf, ni)

    def detect_host(self, xyzi, params=None):
        p = params if params is not None else self.params()
        pts = f32(xyzi).reshape(-1, 4)
        found, co = C.c_int(0), np.zeros(4, np.float32)
        nc, nf, ni = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().lio_ground_detect_host(self.h, ptr(pts, C.c_float), len(pts), C.byref(p), C.byref(found), ptr(co, C.c_float), C.byref(nc), C.byref(nf),
                                           C.byref(ni)), "ground detect_host")
        return self._result(found, co, nc, nf, ni)

    def indices(self, stage):
        """positions in the input cloud of the clipped (0), filtered (1) or inlier (2) points of the last call"""
        n = -lib().lio_ground_download_indices(self.h, int(stage), None, 0)
        out = np.zeros(max(n, 0), np.uint32)
        if n > 0:
            check(int(lib().lio_ground_download_indices(self.h, int(stage), ptr(out, C.c_uint32), n)), "ground indices")
        return out

    def normals(self):
        """n x 3 f32, one per clipped point of the last call"""
        n = -lib().lio_ground_download_normals(self.h, None, 0)
        out = np.zeros((max(n, 0), 3), np.float32)
        if n > 0:
            check(int(lib().lio_ground_download_normals(self.h, ptr(out, C.c_float), n)), "ground normals")
        return out

    def inliers(self):
        """the inlier cloud of the last call, n x 4"""
        n = -lib().lio_ground_download_inliers(self.h, None, 0)
        out = np.zeros((max(n, 0), 4), np.float32)
        if n > 0:
            check(int(lib().lio_ground_download_inliers(self.h, ptr(out, C.c_float), n)), "ground inliers")
        return out

    def draws(self):
        """(triples n x 3 u32, counts n u32 (0xFFFFFFFF: a bad draw), planes n x 4 f32) of every draw the device scored in the last call"""
        n = -lib().lio_ground_download_draws(self.h, None, None, None, 0)
        n = max(n, 0)
        t, c, pl = np.zeros((n, 3), np.uint32), np.zeros(n, np.uint32), np.zeros((n, 4), np.float32)
        if n > 0:
            check(int(lib().lio_ground_download_draws(self.h, ptr(t, C.c_uint32), ptr(c, C.c_uint32), ptr(pl, C.c_float), n)), "ground draws")
        return t, c, pl

    def last_run(self):
        """dict(iterations, skipped, draws_used, winner) of ransac.hpp's loop as the last call replayed it"""
        a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().lio_ground_last_run(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "ground last_run")
        return dict(iterations=a.value, skipped=b.value, draws_used=c.value, winner=d.value)

    def last_times(self):
        """(filter_us, ransac_us): device time of clip + k-NN + normals + filter, and of the RANSAC with the inlier selection"""
        a, b = C.c_double(0), C.c_double(0)
        check(lib().lio_ground_last_times(self.h, C.byref(a), C.byref(b)), "ground times")
        return a.value, b.value


def keyframe_decide(prev, pose, dist_threshold, degree_threshold):
    """lio_keyframe_decide (KeyframeUpdater::is_update, keyframe_updater.hpp:60-75) on the host: (need, must, dx, da)"""
    a, b = f64(prev).reshape(16), f64(pose).reshape(16)
    need, must, dx, da = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0)
    check(lib().lio_keyframe_decide(ptr(a, C.c_double), ptr(b, C.c_double), float(dist_threshold), float(degree_threshold), C.byref(need), C.byref(must),
                                    C.byref(dx), C.byref(da)), "keyframe_decide")
    return bool(need.value), bool(must.value), dx.value, da.value


class KeyFramer:
    """lio_keyframer: the mapping mode's key-frame producer (HdlGraphSlamNodelet::cloud_callback + the two filters of SLAM::runMappingThread)
    on the device; include/lio_hip.h states every rule.  push() takes one odometry frame, pop() hands out the key frames in order."""

    keyframe_decide = staticmethod(keyframe_decide)

    def __init__(self, device=0, **over):
        self.params = self.default_params(**over)
        self.h = lib().lio_keyframer_create(device, C.byref(self.params))
        if not self.h:
            raise capi.LioError("lio_keyframer_create failed: " + lib().lio_last_error().decode())

    @staticmethod
    def default_params(**over):
        p = capi.KeyframerParams()
        lib().lio_keyframer_default_params(C.byref(p))
        for k, v in over.items():
            if not hasattr(p, k):
                raise ValueError(f"lio_keyframer_params has no field {k}")
            setattr(p, k, v)
        return p

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_keyframer_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self):
        check(lib().lio_keyframer_reset(self.h), "keyframer reset")

    def push(self, xyzi, stamp_us, header_stamp_us, odom, delta=None, pose_stamps_us=None, poses=None):
        """one frame: N x 4 points, their stamps (us since the header stamp), the header stamp, the odometry pose (4 x 4) and either the frame's
        delta pose or its pose list (absolute stamps, n x 4 x 4); returns the report as a dict"""
        pts = f32(xyzi).reshape(-1, 4)
        st = np.ascontiguousarray(stamp_us, np.uint32).reshape(-1)
        assert len(st) == len(pts)
        T = f64(odom).reshape(16)
        rep = capi.KeyframeReport()
        if poses is not None and len(poses):
            ps = np.ascontiguousarray(pose_stamps_us, np.uint64).reshape(-1)
            pT = f64(poses).reshape(-1, 16)
            assert len(ps) == len(pT)
            rc = lib().lio_keyframer_push_host(self.h, ptr(pts, C.c_float), ptr(st, C.c_uint32), len(pts), int(header_stamp_us), ptr(T, C.c_double), None,
                                               ptr(ps, C.c_uint64), ptr(pT, C.c_double), len(ps), C.byref(rep))
        else:
            D = f64(delta if delta is not None else np.eye(4)).reshape(16)
            rc = lib().lio_keyframer_push_host(self.h, ptr(pts, C.c_float), ptr(st, C.c_uint32), len(pts), int(header_stamp_us), ptr(T, C.c_double),
                                               ptr(D, C.c_double), None, None, 0, C.byref(rep))
        check(rc, "keyframer push")
        return {k: getattr(rep, k) for k, _ in capi.KeyframeReport._fields_}

    def pending(self):
        return int(lib().lio_keyframer_pending(self.h))

    def pop(self):
        """the oldest key frame: dict(points N x 4 f32, pose 4 x 4 f64, stamp, accum_distance, n_before_filters, n_after_radius); None when none is pending"""
        if self.pending() <= 0:
            return None
        n = -int(lib().lio_keyframer_pop(self.h, None, 0, None, None, None, None, None))
        out = np.zeros((max(n, 1), 4), np.float32)
        pose, stamp, acc, nb, nr = np.zeros(16), C.c_uint64(0), C.c_double(0), C.c_uint32(0), C.c_uint32(0)
        n = check(int(lib().lio_keyframer_pop(self.h, ptr(out, C.c_float), len(out), ptr(pose, C.c_double), C.byref(stamp), C.byref(acc), C.byref(nb),
                                              C.byref(nr))), "keyframer pop")
        return dict(points=out[:n].copy(), pose=pose.reshape(4, 4), stamp=int(stamp.value), accum_distance=acc.value, n_before_filters=int(nb.value),
                    n_after_radius=int(nr.value))

    def radius_outlier(self, xyzi, radius=1.0, min_neighbours=3, key_frame_range=0.0):
        """(kept input indices ascending, rows dropped as not finite, points the radius filter alone keeps): pcl::RadiusOutlierRemoval and, with
        key_frame_range > 0, pointsDistanceFilter(0, range) behind it"""
        pts = f32(xyzi).reshape(-1, 4)
        out, nrad, ndrop = np.zeros(max(len(pts), 1), np.uint32), C.c_uint32(0), C.c_uint32(0)
        n = int(lib().lio_keyframe_filter_host(self.h, ptr(pts, C.c_float), len(pts), float(radius), int(min_neighbours), float(key_frame_range),
                                               ptr(out, C.c_uint32), len(out), C.byref(nrad), C.byref(ndrop)))
        check(n, "radius_outlier")
        return out[:n].copy(), int(ndrop.value), int(nrad.value)

    def fitness(self, xyzi, T):
        """calc_fitness_score of a cloud at pose T against the local map: (score, nr); score is DBL_MAX when nr is 0"""
        pts = f32(xyzi).reshape(-1, 4)
        M = f64(T).reshape(16)
        score, nr = C.c_double(0), C.c_uint32(0)
        check(lib().lio_keyframer_fitness_host(self.h, ptr(pts, C.c_float), len(pts), ptr(M, C.c_double), C.byref(score), C.byref(nr)), "keyframer fitness")
        return score.value, int(nr.value)

    def append_local_map(self, xyzi, T):
        """the local map's append for a host cloud (transform, drop from the front, rebuild the tree); returns the local map's size"""
        pts = f32(xyzi).reshape(-1, 4)
        M = f64(T).reshape(16)
        n = lib().lio_keyframer_append_local_map_host(self.h, ptr(pts, C.c_float), len(pts), ptr(M, C.c_double))
        check(n, "keyframer append_local_map")
        return int(n)

    def local_map(self):
        n = -int(lib().lio_keyframer_download_local_map(self.h, None, 0))
        out = np.zeros((max(n, 0), 4), np.float32)
        if n > 0:
            check(int(lib().lio_keyframer_download_local_map(self.h, ptr(out, C.c_float), n)), "keyframer local_map")
        return out

    def last_times(self):
        """dict of device microseconds per stage of the last call: candidate, fitness, filters, ring"""
        v = [C.c_double(0) for _ in range(4)]
        check(lib().lio_keyframer_last_times(self.h, *[C.byref(x) for x in v]), "keyframer times")
        return dict(candidate_us=v[0].value, fitness_us=v[1].value, filters_us=v[2].value, ring_us=v[3].value)


class BevImage:
    """lio_bev: the bird's-eye intensity image of tools/postprocessing/convert_cloud_image.py on the device (include/lio_hip.h states every
    rule): noise filter by intensity rank, per-pixel means, patch-wise histogram equalisation, 16-bit grey image.  An invalid argument (no
    finite point, a patch below 2 pixels, ...) raises ValueError; device trouble raises LioError."""

    def __init__(self, device=0):
        self.h = lib().lio_bev_create(device)
        if not self.h:
            raise capi.LioError("lio_bev_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_bev_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def _check(rc, what):
        if rc == capi.LIO_E_INVALID:
            raise ValueError(f"{what}: {lib().lio_last_error().decode()}")
        return check(rc, what)

    def preprocess_host(self, xyzi, pixel_per_meter):
        p = f32(xyzi).reshape(-1, 4)
        self._check(lib().lio_bev_preprocess_host(self.h, ptr(p, C.c_float), len(p), float(pixel_per_meter)), "bev preprocess_host")
        return self.info()

    def preprocess_cloud(self, cloud, pixel_per_meter):
        self._check(lib().lio_bev_preprocess_cloud(self.h, cloud.h, float(pixel_per_meter)), "bev preprocess_cloud")
        return self.info()

    def upload_pixels(self, keys, intensity, z, image_w, image_h):
        k = np.ascontiguousarray(keys, np.uint32).reshape(-1)
        i = f32(intensity).reshape(-1)
        zz = None if z is None else f32(z).reshape(-1)
        if len(i) != len(k) or (zz is not None and len(zz) != len(k)):
            raise ValueError("BevImage.upload_pixels: one intensity (and z) per key")
        self._check(lib().lio_bev_upload_pixels(self.h, ptr(k, C.c_uint32), ptr(i, C.c_float), None if zz is None else ptr(zz, C.c_float), len(k),
                                                int(image_w), int(image_h)), "bev upload_pixels")

    def convert(self, window, pixel_per_meter):
        self._check(lib().lio_bev_convert(self.h, float(window), float(pixel_per_meter)), "bev convert")
        return self.image()

    def info(self):
        i = capi.BevInfo()
        check(lib().lio_bev_get_info(self.h, C.byref(i)), "bev info")
        return {k: getattr(i, k) for k, _ in capi.BevInfo._fields_ if k != "reserved"}

    def pixel_coords(self):
        """n x 2 int32 (xs, ys) per input point; (-1, -1) for a point dropped as not finite"""
        n = max(-lib().lio_bev_download_pixel_coords(self.h, None, 0), 0)
        out = np.zeros((n, 2), np.int32)
        if n:
            check(int(lib().lio_bev_download_pixel_coords(self.h, ptr(out, C.c_int32), n)), "bev pixel_coords")
        return out

    def kept(self):
        """input indices of the points the noise filter kept, in ascending (intensity, index) order"""
        n = max(-lib().lio_bev_download_kept(self.h, None, 0), 0)
        out = np.zeros(n, np.uint32)
        if n:
            check(int(lib().lio_bev_download_kept(self.h, ptr(out, C.c_uint32), n)), "bev kept")
        return out

    def pixels(self):
        """(key u32, mean intensity f32, mean z f32) per occupied pixel, keys ascending"""
        n = max(-lib().lio_bev_download_pixels(self.h, None, None, None, 0), 0)
        k, i, z = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        if n:
            check(int(lib().lio_bev_download_pixels(self.h, ptr(k, C.c_uint32), ptr(i, C.c_float), ptr(z, C.c_float), n)), "bev pixels")
        return k, i, z

    def nodes(self):
        """(count u32, step i32 (-1: the node did not run), clip limit f64) per node, xi major"""
        n = max(-lib().lio_bev_download_nodes(self.h, None, None, None, 0), 0)
        c, s, cl = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.float64)
        if n:
            check(int(lib().lio_bev_download_nodes(self.h, ptr(c, C.c_uint32), ptr(s, C.c_int32), ptr(cl, C.c_double), n)), "bev nodes")
        return c, s, cl

    def equalised(self):
        """the f32 value of every occupied pixel before rint"""
        n = max(-lib().lio_bev_download_equalised(self.h, None, 0), 0)
        out = np.zeros(n, np.float32)
        if n:
            check(int(lib().lio_bev_download_equalised(self.h, ptr(out, C.c_float), n)), "bev equalised")
        return out

    def image(self):
        i = self.info()
        out = np.zeros((i["padded_h"], i["padded_w"]), np.uint16)
        n = lib().lio_bev_download_image(self.h, ptr(out, C.c_uint16), out.size)
        check(int(n) if n >= 0 else capi.LIO_E_CAPACITY, "bev image")
        return out

    def last_times(self):
        """(preprocess_us, convert_us): device time of the last preprocess and of the last convert"""
        a, b = C.c_double(0), C.c_double(0)
        check(lib().lio_bev_last_times(self.h, C.byref(a), C.byref(b)), "bev times")
        return a.value, b.value


def bev_grey_table():
    """the 65536-entry grey table of the image (host only)"""
    out = np.zeros(65536, np.uint16)
    lib().lio_bev_grey_table(ptr(out, C.c_uint16))
    return out


def _mix32(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(16))


def ground_draw(seed, j, n):
    """the three distinct indices of draws j (an integer or an array) of a RANSAC run with `seed` over n >= 3 points: include/lio_hip.h's rule
    in numpy integer arithmetic (uint64 holding 32-bit values).  Returns an array (..., 3) of int64."""
    M = np.uint64(0xFFFFFFFF)
    j = np.asarray(j, np.uint64)
    s = _mix32(np.uint64(int(seed) & 0xFFFFFFFF) ^ np.uint64(0x9E3779B9))
    r = [_mix32((s + np.uint64(3) * j + np.uint64(t)) & M) for t in range(3)]
    N = np.uint64(n)
    i0 = (r[0] * N) >> np.uint64(32)
    i1 = (r[1] * (N - np.uint64(1))) >> np.uint64(32)
    i1 = i1 + (i1 >= i0).astype(np.uint64)
    i2 = (r[2] * (N - np.uint64(2))) >> np.uint64(32)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = i2 + (i2 >= lo).astype(np.uint64)
    i2 = i2 + (i2 >= hi).astype(np.uint64)
    return np.stack([i0, i1, i2], -1).astype(np.int64)


def transform_cloud_f32(cloud, M):
    """pcl::transformPointCloud(in, out, M) for XYZ(I) points as PCL 1.9.1 evaluates it in f32: xyz = M(0..2, 0..3) * [x y z 1], left to right"""
    c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4).copy()
    Mf = np.asarray(M, np.float64).astype(np.float32)
    x, y, z = c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy()
    for r in range(3):
        c[:, r] = ((Mf[r, 0] * x + Mf[r, 1] * y) + Mf[r, 2] * z) + Mf[r, 3]
    return c


def transform_cloud_f64(cloud, M):
    """pcl::transformPointCloud(in, out, M) with an Eigen::Matrix4d (overlap_merge.hpp:190-194: the connected frames are moved by the f64 `relative`):
    PCL 1.9.1 evaluates that in double, terms left to right, and casts the result to float (csrc/slam_wrapper.cpp does the same for the static transform)"""
    c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4).copy()
    Md = np.asarray(M, np.float64)
    x, y, z = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64), c[:, 2].astype(np.float64)
    for r in range(3):
        c[:, r] = (((Md[r, 0] * x + Md[r, 1] * y) + Md[r, 2] * z) + Md[r, 3]).astype(np.float32)
    return c


class OverlapMatcher:
    """OverlapDetector::matching of the map-merge / relocalisation tools (slam/localization/include/overlap_merge.hpp:151-211) on the
    device: per candidate the overlap pre-check and the coarse NDT alignment with its fitness score, then the fine GICP alignment of the
    new key frame against the best candidate accumulated with its connected frames, then the final fitness test.  Same constants
    (constructor :45-59): coarse = select_registration_method("NDT_CUDA"), fine = FAST_GICP with max correspondence distance 0.5 and
    transformation epsilon 0.001."""

    def __init__(self, max_points=400_000, device=0, ndt_resolution=1.0, gicp_grid=1.0):
        self.fitness_score_max_range = 25.0
        self.fitness_score_thresh = 1.5
        self.fitness_inlier_thresh = 0.2
        self.max_points = max_points
        self.ndt = Ndt(resolution=ndt_resolution, search_method=7, max_points=max_points, max_voxels=max_points, max_source_points=max_points, device=device)
        self.gicp = Gicp(grid_resolution=gicp_grid, max_points=max_points, k=20, device=device)
        self.scan = Scan(max_raw=max_points, max_ds=max_points, device=device)

    def close(self):
        for o in (self.ndt, self.gicp, self.scan):
            o.close()

    def calc_fitness_score(self, cloud1, cloud2, relpose, max_range):
        """calc_fitness_score(cloud1, cloud2, relpose, max_range) (:214-263) -> (score, inlier ratio)"""
        self.ndt.set_target(overlap_filter(cloud1))
        self.scan.set_ds(cloud2)
        return self.ndt.overlap_score(self.scan, np.asarray(relpose, np.float32).astype(np.float64), max_range)

    def matching(self, new_points, new_odom, candidates, connected=()):
        """new_points / new_odom: the new key frame (cloud, 4 x 4 odometry); candidates: [(points, odom), ...]; connected: frames linked
        to the candidates, [(candidate index, points, odom), ...].  Returns None (no overlap) or dict(best, relative_pose (4 x 4 f32, new
        frame -> accumulated candidate frame ... as the reference returns it), score, coarse=[...])"""
        new_points = f32(new_points).reshape(-1, 4)
        new_odom = f64(new_odom).reshape(4, 4)
        best_score, best, rel, coarse = np.inf, None, None, []
        for ci, (pts, odom) in enumerate(candidates):
            guess = (np.linalg.inv(new_odom) @ f64(odom).reshape(4, 4)).astype(np.float32)
            fit = self.calc_fitness_score(new_points, pts, guess, 1.0)
            if fit[1] < self.fitness_inlier_thresh:
                coarse.append(dict(candidate=ci, skipped="inlier ratio", ratio=fit[1]))
                continue
            self.ndt.set_target(new_points)
            self.scan.set_ds(pts)
            T, conv, it = self.ndt.align(self.scan, guess.astype(np.float64))
            if not conv:
                coarse.append(dict(candidate=ci, skipped="not converged"))
                continue
            Tf = T.astype(np.float32)
            score, _ = self.ndt.fitness_score(self.scan, Tf.astype(np.float64), self.fitness_score_max_range)
            coarse.append(dict(candidate=ci, T=Tf, score=score, iterations=it))
            if score > best_score:
                continue
            best_score, best, rel = score, ci, Tf
        if best is None:
            return None
        # finetune: the best candidate plus its connected frames in the candidate's frame
        bo = f64(candidates[best][1]).reshape(4, 4)
        accum = [f32(candidates[best][0]).reshape(-1, 4)]
        for ci, pts, odom in connected:
            if ci == best:
                accum.append(transform_cloud_f64(pts, np.linalg.inv(bo) @ f64(odom).reshape(4, 4)))
        accum = np.concatenate(accum)
        self.gicp.set_target(accum)
        self.gicp.set_source(new_points)
        g = np.linalg.inv(rel.astype(np.float64)).astype(np.float32)  # Eigen::Isometry3f(relative_pose).inverse()
        T, conv, it = self.gicp.align(g.astype(np.float64), max_corr_dist=0.5, transformation_epsilon=0.001)
        if not conv:
            return None
        relative_pose = T.astype(np.float32)
        score, _ = self.calc_fitness_score(accum, new_points, relative_pose, self.fitness_score_max_range)
        if score > self.fitness_score_thresh:
            return None
        return dict(best=best, relative_pose=relative_pose, score=score, coarse=coarse, fine_iterations=it)


class Comm:
    """one rank of an RCCL communicator (lio_comm_*): the all-gather of per-rank normal equations for joint registration across GPUs"""

    def __init__(self, rank=0, world=1, device=0, uid=None):
        u = (C.c_uint8 * 128)(*uid) if uid is not None else None
        self.h = lib().lio_comm_init(device, rank, world, u)
        if not self.h:
            raise capi.LioError("lio_comm_init failed: " + lib().lio_last_error().decode())
        self.rank, self.world = rank, world

    @staticmethod
    def unique_id():
        u = (C.c_uint8 * 128)()
        check(lib().lio_comm_unique_id(u), "comm unique id")
        return bytes(u)

    def allgather(self, d_local, d_gathered, d_sum=None, stream=None):
        check(lib().lio_allgather_normal_eq(self.h, d_local, d_gathered, d_sum, stream), "allgather")

    def stats(self):
        n, t = C.c_uint64(), C.c_double()
        check(lib().lio_comm_stats(self.h, C.byref(n), C.byref(t)))
        return n.value, t.value

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_comm_destroy(self.h)
        self.h = None

    __del__ = close


class Batch:
    """throughput mode, batched (lio_batch_*): B scans per launch against one resident static map, filter loop on the device"""

    def __init__(self, shared_map, n_slots=8, n_groups=3, max_raw=262144, max_ds=100000, sub_maps=None, comm=None):
        """sub_maps / comm: the joint mode (lio_batch_create_joint) -- every job is registered against `shared_map` AND the further `sub_maps`
        resident on this GPU and, through `comm` (lio.Comm), against the sub-maps the other ranks hold; every rank submits the same job list"""
        self.map = shared_map
        self.n_slots, self.n_groups = n_slots, n_groups
        self._keep = (list(sub_maps or []), comm)
        if sub_maps or comm is not None:
            ms = [shared_map] + list(sub_maps or [])
            hs = (C.c_void_p * len(ms))(*[m.h for m in ms])
            self.h = lib().lio_batch_create_joint(hs, len(ms), comm.h if comm is not None else None, n_slots, n_groups, max_raw, max_ds)
        else:
            self.h = lib().lio_batch_create(shared_map.h, n_slots, n_groups, max_raw, max_ds)
        if not self.h:
            raise capi.LioError("lio_batch_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_batch_destroy(self.h)
        self.h = None

    __del__ = close

    def set_gather_hook(self, fn, rank, world):
        """lio_batch_set_gather_hook: fn(d_local: int, d_gathered: int, n_records: int, stream: int) -> int (0 = ok) moves the round's records
        between the ranks instead of RCCL (lsd_amd.dist.RecordsAllGatherHost: gloo, two ranks on one GPU in the tests)"""

        def _cb(_ctx, d_local, d_gathered, n, stream):
            try:
                return int(fn(int(d_local or 0), int(d_gathered or 0), int(n), int(stream or 0)) or 0)
            except Exception:  # nothing may propagate through the C frames
                import traceback

                traceback.print_exc()
                return -1

        self._gather = capi.GATHER_FN(_cb)  # keep the trampoline alive
        check(lib().lio_batch_set_gather_hook(self.h, self._gather, None, int(rank), int(world)), "set_gather_hook")

    def exchange_stats(self):
        """lio_batch_exchange_stats: the all-gather of a joint round's downsampled clouds -- points per slot chunk in force, jobs that ran again because
        their cloud was cut, bytes one rank contributes per round (zeros for one rank / LIO_JOINT_SPLIT_DS=0)"""
        cap, again, nbytes = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().lio_batch_exchange_stats(self.h, C.byref(cap), C.byref(again), C.byref(nbytes)))
        return {"chunk_points": cap.value, "jobs_rerun": again.value, "bytes_per_rank_and_round": nbytes.value}

    def enable_kernel_timing(self, on=True):
        check(lib().lio_batch_enable_kernel_timing(self.h, int(on)))

    def kernel_times(self, reset=True):
        t = capi.BatchTimes()
        check(lib().lio_batch_kernel_times(self.h, C.byref(t), int(reset)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def engine(self, group, slot):
        """the engine behind a slot (borrowed: its scan buffers / neighbour cache, the pass log of a host continuation)"""
        h = lib().lio_batch_engine(self.h, group, slot)
        if not h:
            raise capi.LioError("no such slot")
        e = Engine.__new__(Engine)
        e.h = h
        e._own = False
        e.map = self.map
        e.scan = Scan(max_ds=100000, _borrow=lib().lio_engine_scan(h))
        return e

    def process(self, jobs):
        """jobs: list of dicts {dptr, n, t, state (26,), cov (23,23)}; returns (rc, list of result dicts) like process_batch"""
        return process_batch(None, jobs, batch=self)


JOB_KEEP_CACHE = 1  # LIO_JOB_KEEP_CACHE of include/lio_hip.h
JOB_IDLE = 2        # LIO_JOB_IDLE: the session has no scan this round (lio_batch_sequences_step)
JOB_HOST_RAW = 4    # LIO_JOB_HOST_RAW: "dptr" is a HOST address (pinned: PinnedCloud); the library copies it to HBM on the round's stream


class PinnedCloud:
    """a cloud in page-locked host memory (lio_pinned_alloc): .array is an (n, 4) float32 view to fill, .ptr the address for a JOB_HOST_RAW job"""

    def __init__(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
        self.n = len(pts)
        self.nbytes = max(pts.nbytes, 16)
        self.ptr = lib().lio_pinned_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError((lib().lio_last_error() or b'').decode())
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_float)), shape=(max(self.n, 1), 4))[: self.n]
        self.array[...] = pts

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                self.array = None
                lib().lio_pinned_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


class SequenceBatch:
    """throughput mode WITH map_incremental (lio_batch_create_sequences): n_groups x n_slots independent SLAM sessions, one per slot, each with its
    own map; step() registers the next scan of every session and inserts it into the session's map in one submission per group"""

    def __init__(self, n_slots=8, n_groups=1, resolution=0.5, stencil=19, max_points=2_000_000, max_voxels=1_000_000, max_raw=262144, max_ds=100000, device=0):
        self.n_slots, self.n_groups = n_slots, n_groups
        self.n = n_slots * n_groups
        self.h = lib().lio_batch_create_sequences(device, resolution, stencil, max_points, max_voxels, n_slots, n_groups, max_raw, max_ds)
        if not self.h:
            raise capi.LioError("lio_batch_create_sequences failed: " + lib().lio_last_error().decode())
        self.arr = (capi.ScanJob * self.n)()
        self.states_in = np.zeros((self.n, STATE_DIM))
        self.covs_in = np.zeros((self.n, 23 * 23))
        self.states_out = np.zeros((self.n, STATE_DIM))
        self.covs_out = np.zeros((self.n, 23 * 23))
        for i in range(self.n):
            a = self.arr[i]
            a.state_in = self.states_in[i].ctypes.data_as(C.POINTER(C.c_double))
            a.cov_in = self.covs_in[i].ctypes.data_as(C.POINTER(C.c_double))
            a.state_out = self.states_out[i].ctypes.data_as(C.POINTER(C.c_double))

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_batch_destroy(self.h)
        self.h = None

    __del__ = close

    def engine(self, session):
        """the engine that owns session `session`'s map and file-scope state (borrowed)"""
        h = lib().lio_batch_engine(self.h, session // self.n_slots, session % self.n_slots)
        if not h:
            raise capi.LioError("no such session")
        e = Engine.__new__(Engine)
        e.h = h
        e._own = False
        e.map = Map(_borrow=lib().lio_engine_map(h))
        e.scan = Scan(max_ds=100000, _borrow=lib().lio_engine_scan(h))
        return e

    def enable_kernel_timing(self, on=True):
        check(lib().lio_batch_enable_kernel_timing(self.h, int(on)))

    def kernel_times(self, reset=True):
        t = capi.BatchTimes()
        check(lib().lio_batch_kernel_times(self.h, C.byref(t), int(reset)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def fastlio_main(self):
        """lio_batch_fastlio_main: one fastlio_main per session (their engines carry the front half: engine(s).fastlio_init, fastlio_imu_enqueue,
        fastlio_pcl_enqueue...), the registrations of all sessions as one round; returns (rc, per-session return codes)"""
        if not hasattr(self, "_fl_rc"):
            self._fl_rc = (C.c_int * self.n)()
        rc = lib().lio_batch_fastlio_main(self.h, self._fl_rc)
        return rc, list(self._fl_rc)

    def load(self, jobs):
        """jobs: one entry per session -- None (idle this round) or a dict {dptr, n, t, state (26,), cov (23,23)}"""
        assert len(jobs) == self.n
        for i, j in enumerate(jobs):
            a = self.arr[i]
            if j is None:
                a.flags = JOB_IDLE
                a.d_raw, a.n_raw = None, 0
                continue
            a.flags = 0
            a.d_raw = j["dptr"]
            a.n_raw = j["n"]
            a.lidar_beg_time = float(j["t"])
            self.states_in[i] = f64(j["state"])
            self.covs_in[i] = f64(j["cov"]).reshape(-1)

    def run(self):
        """the C call alone (on what load() marshalled)"""
        return lib().lio_batch_sequences_step(self.h, self.arr, self.n, self.covs_out.ctypes.data_as(C.POINTER(C.c_double)))

    def step(self, jobs):
        """returns (rc, list of result dicts -- None for an idle session)"""
        self.load(jobs)
        rc = self.run()
        a = self.arr
        res = [None if jobs[i] is None else dict(rc=a[i].rc, n_ds=a[i].n_ds, n_pass=a[i].n_pass, n_knn_pass=a[i].n_knn_pass, state=self.states_out[i].copy(),
                                                  cov=self.covs_out[i].reshape(23, 23).copy()) for i in range(self.n)]
        return rc, res



class PreparedJobs:
    """a job list marshalled once into the C ABI's lio_scan_job array (so that a timed region can be the one C call and nothing else)"""

    def __init__(self, jobs):
        n = len(jobs)
        self.n = n
        self.arr = (capi.ScanJob * n)()
        self.outs = np.zeros((n, STATE_DIM))
        self._keep = []
        cache = {}
        for i, j in enumerate(jobs):
            key = (id(j["state"]), id(j["cov"]))
            if key not in cache:  # the same arrays handed in many times (a repeated list) are converted once
                cache[key] = (f64(j["state"]), f64(j["cov"]).reshape(-1))
                self._keep.append(cache[key])
            st, cv = cache[key]
            a = self.arr[i]
            a.d_raw = j["dptr"]
            a.n_raw = j["n"]
            a.flags = int(j.get("flags", 0))  # 0: an independent scan (the slot forgets its neighbour cache first); JOB_KEEP_CACHE: one of a sequence
            a.lidar_beg_time = float(j["t"])
            a.state_in = ptr(st, C.c_double)
            a.cov_in = ptr(cv, C.c_double)
            a.state_out = self.outs[i].ctypes.data_as(C.POINTER(C.c_double))

    def results(self):
        a = self.arr
        return [dict(rc=a[i].rc, n_ds=a[i].n_ds, n_pass=a[i].n_pass, n_knn_pass=a[i].n_knn_pass, state=self.outs[i]) for i in range(self.n)]


def run_prepared(prep, engines=None, batch=None):
    """the C call alone: lio_batch_process (batch=) or lio_engines_process_batch (engines=) on a PreparedJobs; returns its return code"""
    if batch is not None:
        return lib().lio_batch_process(batch.h, prep.arr, prep.n)
    hs = (C.c_void_p * len(engines))(*[e.h for e in engines])
    return lib().lio_engines_process_batch(hs, len(engines), prep.arr, prep.n)


def process_batch(engines, jobs, batch=None):
    """register independent scans concurrently (C++ worker threads, one per engine; see lio_engines_process_batch) or, with
    batch=, through the batched device-resident engine (lio_batch_process).
    jobs: list of dicts {dptr, n, t, state (26,), cov (23,23)}; returns (rc, list of result dicts)"""
    prep = PreparedJobs(jobs)
    rc = run_prepared(prep, engines=engines, batch=batch)
    return rc, prep.results()


def state_boxplus(s, d):
    s, d = f64(s), f64(d)
    o = np.zeros(STATE_DIM)
    lib().lio_state_boxplus(ptr(s, C.c_double), ptr(d, C.c_double), ptr(o, C.c_double))
    return o


def state_boxminus(a, b):
    a, b = f64(a), f64(b)
    o = np.zeros(DOF)
    lib().lio_state_boxminus(ptr(a, C.c_double), ptr(b, C.c_double), ptr(o, C.c_double))
    return o


def state_predict(s, P, dt, Q12, acc, gyro):
    """one esekf::predict step on the host (no GPU needed): returns (state26, P 23x23)"""
    s, P, q, a, g = f64(s), f64(P).reshape(-1), f64(Q12), f64(acc), f64(gyro)
    assert s.size == STATE_DIM and P.size == 529 and q.size == 12
    so, Po = np.zeros(STATE_DIM), np.zeros(529)
    check(lib().lio_state_predict(ptr(s, C.c_double), ptr(P, C.c_double), float(dt), ptr(q, C.c_double), ptr(a, C.c_double), ptr(g, C.c_double),
                                  ptr(so, C.c_double), ptr(Po, C.c_double)))
    return so, Po.reshape(23, 23)


NO_EFFECTIVE_POINTS = "no effective points"  # a model's answer for a pass in which h_share_model_geometric returns early (laserMapping.cpp:888-893)


def make_meas_fn(model):
    """wrap model(state26, converge) -> (rows (n, 6), h (n,)), None (the pass is invalid) or NO_EFFECTIVE_POINTS (the point-to-plane part found
    nothing: the rows of the previous pass survive in the copied struct, laserMapping.cpp:991) as the C measurement callback of lio_eskf_update_cb"""
    def _cb(ctx, s26, converge, n_out, rows, h, cap):
        r = model(np.ctypeslib.as_array(s26, shape=(STATE_DIM,)).copy(), bool(converge))
        if r is None:
            return 0
        if isinstance(r, str) and r == NO_EFFECTIVE_POINTS:
            n_out[0] = 0
            return 2
        R, H = np.asarray(r[0], np.float64).reshape(-1, 6), np.asarray(r[1], np.float64).ravel()
        n = len(H)
        assert n <= cap and len(R) == n
        np.ctypeslib.as_array(rows, shape=(cap * 6,))[:n * 6] = R.ravel()
        np.ctypeslib.as_array(h, shape=(cap,))[:n] = H
        n_out[0] = n
        return 1
    return capi.MEAS_FN(_cb)


def eskf_update(s, P, R, model, max_iter=4, cap=4096):
    """one iterated ESKF update on the host filter with a Python measurement model (see make_meas_fn)"""
    s, P = f64(s), f64(P).reshape(-1)
    so, Po = np.zeros(STATE_DIM), np.zeros(529)
    fn = make_meas_fn(model)
    check(lib().lio_eskf_update_cb(ptr(s, C.c_double), ptr(P, C.c_double), float(R), max_iter, fn, None, cap, ptr(so, C.c_double), ptr(Po, C.c_double)))
    return so, Po.reshape(23, 23)


def eskf_update_ws(s, P, R, model, ins_vel, degenerate=False, max_iter=4, cap=4096):
    """eskf_update with the wheel-speed rows (laserMapping.cpp:794-811) appended to the model's rows in every pass"""
    s, P, v = f64(s), f64(P).reshape(-1), f64(ins_vel)
    so, Po = np.zeros(STATE_DIM), np.zeros(529)
    fn = make_meas_fn(model)
    check(lib().lio_eskf_update_ws_cb(ptr(s, C.c_double), ptr(P, C.c_double), float(R), max_iter, fn, None, cap, ptr(v, C.c_double), int(degenerate),
                                      ptr(so, C.c_double), ptr(Po, C.c_double)))
    return so, Po.reshape(23, 23)


def sums_of_rows(rows, h):
    """the 29 numbers a device linearisation hands the filter: J^T J upper triangle row by row, J^T h, sum |r|, N_eff"""
    rows, h = np.asarray(rows, np.float64).reshape(-1, 6), np.asarray(h, np.float64).ravel()
    JtJ, Jth = rows.T @ rows, rows.T @ h
    return np.concatenate([[JtJ[a, b] for a in range(6) for b in range(a, 6)], Jth, [np.abs(h).sum(), float(len(h))]])


def eskf_update_sums(s, P, R, model, max_iter=4, degenerate_detect=False):
    """the DEVICE-resident form of the iterated update (csrc/eskf_dev.h compiled for the host) with a Python model:
    model(state26, converge) -> (rows (n, 6), h (n,)) or None.  Returns (state26, P, logs, status)."""
    s, P = f64(s), f64(P).reshape(-1)
    so, Po = np.zeros(STATE_DIM), np.zeros(529)
    last = {}

    def _sums(ctx, s26, converge, acc):
        r = model(np.ctypeslib.as_array(s26, shape=(STATE_DIM,)).copy(), bool(converge))
        if r is None:
            return 0
        last["rows"] = np.asarray(r[0], np.float64).reshape(-1, 6)
        np.ctypeslib.as_array(acc, shape=(29,))[:] = sums_of_rows(r[0], r[1])
        return 1

    def _deg(ctx, V, cs):  # laserMapping.cpp:946-964 on the rows of the last evaluation
        Vm = np.ctypeslib.as_array(V, shape=(9,)).reshape(3, 3)
        n = last["rows"][:, :3]
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        d = np.abs(n @ Vm).astype(np.float32).astype(np.float64)
        out = np.ctypeslib.as_array(cs, shape=(6,))
        out[:3] = np.where(d > np.float32(0.1736), d, 0).sum(0)
        out[3:] = np.where(d > np.float32(0.7070), d, 0).sum(0)

    f1, f2 = capi.SUMS_FN(_sums), capi.DEG_FN(_deg)
    logs = (capi.PassLog * 8)()
    status = C.c_int(0)
    n = check(lib().lio_eskf_update_sums_cb(ptr(s, C.c_double), ptr(P, C.c_double), float(R), max_iter, int(degenerate_detect), f1, f2, None,
                                            ptr(so, C.c_double), ptr(Po, C.c_double), logs, 8, C.byref(status)), "eskf_update_sums")
    out = [dict(knn=l.knn, n_eff=l.n_eff, valid=l.valid, degenerate=l.degenerate, sum_abs_res=l.sum_abs_res, JtJ=np.array(l.JtJ).reshape(6, 6),
                Jtr=np.array(l.Jtr), dx=np.array(l.dx)) for l in logs[:n]]
    return so, Po.reshape(23, 23), out, status.value


class PoseEstimator:
    """hdl_localization::PoseEstimator over the device matcher: 23-state UKF (host, f32) + lio_ndt_align.
    Stamps in microseconds, quaternions (w, x, y, z), as in the reference."""

    def __init__(self, pos, quat_wxyz, stamp_us=0, imu_ext=np.eye(4), cool_time=1.0):
        a, b, c = f32(imu_ext).reshape(-1), f32(pos), f32(quat_wxyz)
        self.h = lib().lio_pose_estimator_create(ptr(a, C.c_float), int(stamp_us), ptr(b, C.c_float), ptr(c, C.c_float), float(cool_time))
        if not self.h:
            raise capi.LioError("lio_pose_estimator_create failed")

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_pose_estimator_destroy(self.h)
        self.h = None

    __del__ = close

    def predict(self, stamp_us, acc=None, gyro=None):
        if acc is None:
            return check(lib().lio_pose_estimator_predict(self.h, int(stamp_us), None, None), "predict")
        a, g = f32(acc), f32(gyro)
        return check(lib().lio_pose_estimator_predict(self.h, int(stamp_us), ptr(a, C.c_float), ptr(g, C.c_float)), "predict")

    def match(self, ndt, scan, params=None):
        """returns (ok, observation (7,), LM iterations)"""
        obs = np.zeros(7, np.float32)
        it = C.c_int(0)
        p = params
        if p is None:
            p = capi.NdtParams()
            lib().lio_ndt_default_params(C.byref(p))
        ok = check(lib().lio_pose_estimator_match(self.h, ndt.h, scan.h, C.byref(p), ptr(obs, C.c_float), C.byref(it)), "match")
        return bool(ok), obs, it.value

    @staticmethod
    def _gps(gps):
        """gps: None or (T 4x4, precision, dimension) -> pointer to a lio_gps_observation (kept alive by the caller's frame)"""
        if gps is None:
            return None, None
        g = capi.GpsObservation()
        T = f64(gps[0]).reshape(16)
        for i in range(16):
            g.T[i] = T[i]
        g.precision, g.dimension = float(gps[1]), int(gps[2])
        return g, C.byref(g)

    def guess(self, gps=None):
        """the pose the matcher starts from: the filter's, fused with the GNSS observation when there is one"""
        keep, gp = self._gps(gps)
        T = np.zeros(16, np.float32)
        check(lib().lio_pose_estimator_guess(self.h, gp, ptr(T, C.c_float)), "guess")
        return T.reshape(4, 4)

    def observe(self, init_guess, aligned, converged=True, gps=None):
        """what match() makes of the matcher's answer: (ok, observation (7,), observation covariance (7, 7))"""
        keep, gp = self._gps(gps)
        a, b = f32(init_guess).reshape(16), f32(aligned).reshape(16)
        obs, cov = np.zeros(7, np.float32), np.zeros(49, np.float32)
        ok = check(lib().lio_pose_estimator_observe(self.h, ptr(a, C.c_float), ptr(b, C.c_float), int(converged), gp, ptr(obs, C.c_float), ptr(cov, C.c_float)), "observe")
        return bool(ok), obs, cov.reshape(7, 7)

    def match_gps(self, ndt, scan, gps, params=None):
        keep, gp = self._gps(gps)
        obs, cov, it = np.zeros(7, np.float32), np.zeros(49, np.float32), C.c_int(0)
        p = params
        if p is None:
            p = capi.NdtParams()
            lib().lio_ndt_default_params(C.byref(p))
        ok = check(lib().lio_pose_estimator_match_gps(self.h, ndt.h, scan.h, C.byref(p), gp, ptr(obs, C.c_float), ptr(cov, C.c_float), C.byref(it)), "match_gps")
        return bool(ok), obs, cov.reshape(7, 7), it.value

    def match_gps_only(self, gps):
        keep, gp = self._gps(gps)
        obs, cov = np.zeros(7, np.float32), np.zeros(49, np.float32)
        ok = check(lib().lio_pose_estimator_match_gps_only(self.h, gp, ptr(obs, C.c_float), ptr(cov, C.c_float)), "match_gps_only")
        return bool(ok), obs, cov.reshape(7, 7)

    def get_timed_pose(self, stamp_us, acc_g, gyro_dps):
        """one INS sample (g, deg/s) -> (accepted, pose 4x4 at that sample); extends the state queue that correct() re-predicts"""
        a, g, T = f64(acc_g), f64(gyro_dps), np.zeros(16)
        ok = check(lib().lio_pose_estimator_get_timed_pose(self.h, int(stamp_us), ptr(a, C.c_double), ptr(g, C.c_double), ptr(T, C.c_double)), "get_timed_pose")
        return bool(ok), T.reshape(4, 4)

    def predict_nostate(self, stamp_us):
        T = np.zeros(16)
        check(lib().lio_pose_estimator_predict_nostate(self.h, int(stamp_us), ptr(T, C.c_double)), "predict_nostate")
        return T.reshape(4, 4)

    def correct(self, stamp_us, observation):
        z = f32(observation)
        check(lib().lio_pose_estimator_correct(self.h, int(stamp_us), ptr(z, C.c_float)), "correct")

    def get(self):
        m, c = np.zeros(23, np.float32), np.zeros(529, np.float32)
        check(lib().lio_pose_estimator_get(self.h, ptr(m, C.c_float), ptr(c, C.c_float)))
        return m, c.reshape(23, 23)

    def set(self, mean=None, cov=None):
        m = f32(mean) if mean is not None else None
        c = f32(cov).reshape(-1) if cov is not None else None
        check(lib().lio_pose_estimator_set(self.h, ptr(m, C.c_float) if m is not None else None, ptr(c, C.c_float) if c is not None else None))

    def matrix(self):
        T = np.zeros(16, np.float32)
        check(lib().lio_pose_estimator_matrix(self.h, ptr(T, C.c_float)))
        return T.reshape(4, 4)


class LocalMap:
    """Localization::runUpdateLocalMap on the device: key-frame clouds resident in HBM, local map = gather + VoxelGrid + NDT target"""

    def __init__(self, max_total_points=20_000_000, max_local_points=200_000, max_keyframe_points=200_000, device=0):
        self.h = lib().lio_localmap_create(device, max_total_points, max_local_points, max_keyframe_points)
        if not self.h:
            raise capi.LioError("lio_localmap_create failed: " + lib().lio_last_error().decode())
        self._cap = max_local_points + max_keyframe_points

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_localmap_destroy(self.h)
        self.h = None

    __del__ = close

    def add_keyframe(self, world_xyzi, position):
        p, c = f32(world_xyzi).reshape(-1, 4), f32(position)
        return check(lib().lio_localmap_add_keyframe(self.h, ptr(p, C.c_float), len(p), ptr(c, C.c_float)), "add_keyframe")

    def update(self, ndt, pose_xyz, update_distance=10.0, radius=30.0, key_frame_distance=1.0, leaf=0.2):
        """returns (code, key frames used, points in the new target); code as lio_localmap_update"""
        x = f64(pose_xyz)
        nk, npts = C.c_int(0), C.c_uint32(0)
        rc = check(lib().lio_localmap_update(self.h, ndt.h, ptr(x, C.c_double), float(update_distance), float(radius), float(key_frame_distance), float(leaf),
                                             C.byref(nk), C.byref(npts)), "localmap update")
        return rc, nk.value, npts.value

    def download(self):
        out = np.zeros((self._cap, 4), np.float32)
        n = check(lib().lio_localmap_download(self.h, ptr(out, C.c_float), self._cap))
        return out[:n].copy()

    # ---- the operator's pose hint (GlobalLocalization::getEstimatePose) ----
    def nearest(self, xy, k=5):
        """(ids, d2) of the min(k, frames) key frames nearest (x, y), rising (d2, id); d2 in f32 as the C entry computes it"""
        x = f64(xy)
        ids, d2 = np.zeros(max(int(k), 1), np.int32), np.zeros(max(int(k), 1), np.float32)
        n = check(lib().lio_localmap_nearest(self.h, ptr(x, C.c_double), int(k), ptr(ids, C.c_int32), ptr(d2, C.c_float)), "localmap nearest")
        return ids[:n].copy(), d2[:n].copy()

    def gather(self, ids):
        """the named key frames back to back in a device buffer -> (points, mean z by the chunked sum)"""
        i = np.ascontiguousarray(ids, np.int32).reshape(-1)
        n, z = C.c_uint32(0), C.c_double(0)
        check(lib().lio_localmap_gather(self.h, ptr(i, C.c_int32), len(i), C.byref(n), C.byref(z)), "localmap gather")
        return n.value, z.value

    def gather_device(self):
        """(device address, points) of the last gather"""
        n = C.c_uint32(0)
        p = lib().lio_localmap_gather_device(self.h, C.byref(n))
        return p, n.value

    def download_gather(self):
        p, n = self.gather_device()
        out = np.zeros((max(n, 1), 4), np.float32)
        m = check(lib().lio_localmap_download_gather(self.h, ptr(out, C.c_float), len(out)), "localmap download_gather")
        return out[:m].copy()

    def z_mean(self, d_ptr, n):
        z = C.c_double(0)
        check(lib().lio_localmap_z_mean(self.h, C.c_void_p(d_ptr), int(n), C.byref(z)), "localmap z_mean")
        return z.value

    def store_frame(self, slot, d_ptr, n):
        check(lib().lio_localmap_store_frame(self.h, int(slot), C.c_void_p(d_ptr), int(n)), "localmap store_frame")

    def frame(self, slot):
        n = C.c_uint32(0)
        p = lib().lio_localmap_frame(self.h, int(slot), C.byref(n))
        return p, n.value

    def estimate_pose(self, gicp, d_source, n_source, hint):
        """lio_localmap_estimate_pose -> (out_T 4 x 4, report dict)"""
        h, out, rep = f64(hint).reshape(4, 4), np.zeros((4, 4)), capi.EstimateReport()
        check(lib().lio_localmap_estimate_pose(self.h, gicp.h, C.c_void_p(d_source), int(n_source), ptr(h, C.c_double), C.byref(rep), ptr(out, C.c_double)),
              "localmap estimate_pose")
        r = {k: getattr(rep, k) for k, _ in capi.EstimateReport._fields_ if k not in ("ids", "guess")}
        r["ids"] = [int(v) for v in rep.ids[:rep.n_ids]]
        r["guess"] = np.array(rep.guess).reshape(4, 4)
        return out, r


class ColourMap:
    """lio_render: the road-surface colour map of slam/localization/map_render on the device (include/lio_hip.h states every rule): floor
    points of a frame enter 0.2 m voxels, every stored point of the touched voxels is projected into the frame's camera images, a z-buffer
    and a 9 x 9 depth test decide what is seen, and the seen points blend a bilinear sample into their colour.  `frame` returns "skipped",
    "no_floor" or "rendered"; an invalid argument raises ValueError, a frame that does not fit LioError (the map is unchanged)."""

    OUTCOME = {capi.RENDER_SKIPPED: "skipped", capi.RENDER_NO_FLOOR: "no_floor", capi.RENDER_DONE: "rendered"}

    def __init__(self, max_voxels=1 << 20, max_points=1 << 24, device=0, active=True):
        self.h = lib().lio_render_create(device, int(max_voxels), int(max_points))
        if not self.h:
            raise capi.LioError("lio_render_create failed: " + lib().lio_last_error().decode())
        self.names = []
        self.set_active(active)

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_render_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def _check(rc, what):
        if rc == capi.LIO_E_INVALID:
            raise ValueError(f"{what}: {lib().lio_last_error().decode()}")
        return check(rc, what)

    def set_cameras(self, cameras, lidar_static=None):
        """cameras: {name: (K, extrinsic)} with K = (fx, fy, cx, cy) or a 3 x 3 matrix and a 4 x 4 extrinsic; lidar_static: 4 x 4 or None"""
        names = list(cameras)
        intr, ext = np.zeros((len(names), 4)), np.zeros((len(names), 16))
        for i, n in enumerate(names):
            K, E = cameras[n]
            K = np.asarray(K, np.float64)
            intr[i] = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.ndim == 2 else K.ravel()[:4]
            ext[i] = f64(E).reshape(16)
        arr = (C.c_char_p * max(len(names), 1))(*[str(n).encode() for n in names])
        ls = f64(lidar_static).reshape(16) if lidar_static is not None else None
        self._check(lib().lio_render_set_cameras(self.h, len(names), arr, ptr(intr, C.c_double), ptr(ext, C.c_double),
                                                 ptr(ls, C.c_double) if ls is not None else None), "render set_cameras")
        self.names = [str(n) for n in names]

    def set_active(self, active):
        check(lib().lio_render_set_active(self.h, int(bool(active))), "render set_active")

    def frame(self, xyzi, pose, images=None, use_ground=True, seed=0):
        """images: {camera name: (bgr image rows x cols x 3 u8, 4 x 4 pose)}"""
        p = f32(xyzi).reshape(-1, 4)
        T = f64(pose).reshape(16)
        images = images or {}
        buf, keep = (capi.RenderImage * max(len(images), 1))(), []
        for i, (name, (img, ipose)) in enumerate(images.items()):
            a = np.asarray(img)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("ColourMap.frame: an image must be rows x cols x 3 (BGR); the I420 conversion of imageCvtColor is out of scope")
            if str(name) not in self.names:
                raise ValueError(f"ColourMap.frame: no camera named {name}")
            a = np.ascontiguousarray(a, np.uint8)
            keep.append(a)
            buf[i].camera, buf[i].rows, buf[i].cols, buf[i].bgr = self.names.index(str(name)), a.shape[0], a.shape[1], a.ctypes.data
            buf[i].pose[:] = list(f64(ipose).reshape(16))
        rc = self._check(lib().lio_render_frame(self.h, ptr(p, C.c_float), len(p), ptr(T, C.c_double), int(bool(use_ground)), int(seed) & 0xFFFFFFFF, buf,
                                                len(images)), "render frame")
        return self.OUTCOME[rc]

    def clear(self):
        check(lib().lio_render_clear(self.h), "render clear")

    def size(self):
        """(voxels, points) the map holds"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib().lio_render_size(self.h, C.byref(a), C.byref(b)), "render size")
        return a.value, b.value

    def colour_map(self):
        """getColorMap as pointcloud_to_numpy(PointCloudRGB) returns it: n x 4 f32, the last column r << 16 | g << 8 | b as f32 bits"""
        n = max(-int(lib().lio_render_download(self.h, None, 0)), 0)
        out = np.zeros((n, 4), np.float32)
        if n:
            check(int(lib().lio_render_download(self.h, ptr(out, C.c_float), n)), "render download")
        return out

    def voxels(self):
        """dict box (n x 3 i32), hits, counts (u32) in voxel number order"""
        n = self.size()[0]
        box, hits, cnt = np.zeros((n, 3), np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        if n:
            check(int(lib().lio_render_download_voxels(self.h, ptr(box, C.c_int32), ptr(hits, C.c_uint32), ptr(cnt, C.c_uint32), n)), "render voxels")
        return dict(box=box, hits=hits, counts=cnt)

    def points(self):
        """dict xyz (n x 3 f32), voxel (u32), rgb (n x 3 f32), score, depth (f32) in serial number order"""
        n = self.size()[1]
        xyz, vox, rgb = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros((n, 3), np.float32)
        score, depth = np.zeros(n, np.float32), np.zeros(n, np.float32)
        if n:
            check(int(lib().lio_render_download_points(self.h, ptr(xyz, C.c_float), ptr(vox, C.c_uint32), ptr(rgb, C.c_float), ptr(score, C.c_float),
                                                       ptr(depth, C.c_float), n)), "render points")
        return dict(xyz=xyz, voxel=vox, rgb=rgb, score=score, depth=depth)

    def last_image(self):
        """dict depth (rows x cols f32, -1: no owner), owner (i32 serial, -1), valid (u8) of the last image of the last rendered frame"""
        r, c = C.c_int(0), C.c_int(0)
        n = max(-int(lib().lio_render_download_last_image(self.h, None, None, None, 0, C.byref(r), C.byref(c))), 0)
        d, o, v = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        if n:
            check(int(lib().lio_render_download_last_image(self.h, ptr(d, C.c_float), ptr(o, C.c_int32), ptr(v, C.c_uint8), n, C.byref(r), C.byref(c))),
                  "render last_image")
        shape = (r.value, c.value)
        return dict(depth=d.reshape(shape), owner=o.reshape(shape), valid=v.reshape(shape))

    def last_times(self):
        v = [C.c_double(0) for _ in range(3)]
        check(lib().lio_render_last_times(self.h, *[C.byref(x) for x in v]), "render times")
        return dict(insert_us=v[0].value, image_us=v[1].value, finish_us=v[2].value)


def rtk_fix(stamp_us=0, latitude=0.0, longitude=0.0, altitude=0.0, heading=0.0, pitch=0.0, roll=0.0, precision=100.0, dimension=2):
    """a lio_rtk_fix (degrees, metres; the defaults of the reference's RTKType)"""
    return capi.RtkFix(int(stamp_us), float(latitude), float(longitude), float(altitude), float(heading), float(pitch), float(roll), float(precision),
                       int(dimension), 0)


def _fix(f):
    return f if isinstance(f, capi.RtkFix) else rtk_fix(**f)


def grid_convergence(longitude0, lat, lon):
    return lib().lio_grid_convergence(float(longitude0), float(lat), float(lon))


def transform_from_rpyt(x, y, z, yaw, pitch, roll):
    T = np.zeros((4, 4))
    lib().lio_transform_from_rpyt(float(x), float(y), float(z), float(yaw), float(pitch), float(roll), ptr(T, C.c_double))
    return T


def interpolate_transform(pre, nxt, ratio):
    a, b, T = f64(pre).reshape(4, 4), f64(nxt).reshape(4, 4), np.zeros((4, 4))
    lib().lio_interpolate_transform(ptr(a, C.c_double), ptr(b, C.c_double), float(ratio), ptr(T, C.c_double))
    return T


def update_origin(origin_from, origin_to, poses=None, xyz=None):
    """graph_update_origin's coordinate change: poses ((n, 4, 4)) and points ((m, 3)) of a map recorded under origin_from, expressed under
    origin_to -> (poses, xyz), f64 copies; rotations are not touched.  An origin is a fix, or (latitude, longitude, altitude)"""
    a, b = [o if isinstance(o, (capi.RtkFix, dict)) else dict(latitude=o[0], longitude=o[1], altitude=o[2]) for o in (origin_from, origin_to)]
    P = np.array(poses if poses is not None else np.zeros((0, 4, 4)), np.float64).reshape(-1, 4, 4)
    X = np.array(xyz if xyz is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3)
    check(lib().lio_update_origin(C.byref(_fix(a)), C.byref(_fix(b)), ptr(P, C.c_double), len(P), ptr(X, C.c_double), len(X)), "update_origin")
    return P, X


class Utm:
    """lio_utm: the reference's UTMProjector, host only.  The zone is fixed by the first call (zone is -1 until then)."""

    def __init__(self, zone_width=6):
        self.h = lib().lio_utm_create(int(zone_width))
        if not self.h:
            raise capi.LioError("lio_utm_create failed")

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_utm_destroy(self.h)
        self.h = None

    __del__ = close

    @property
    def zone(self):
        return lib().lio_utm_zone(self.h)

    def forward(self, lat, lon):
        x, y = C.c_double(0), C.c_double(0)
        check(lib().lio_utm_forward(self.h, float(lat), float(lon), C.byref(x), C.byref(y)), "utm forward")
        return x.value, y.value

    def inverse(self, x, y):
        lat, lon = C.c_double(0), C.c_double(0)
        check(lib().lio_utm_inverse(self.h, float(x), float(y), C.byref(lat), C.byref(lon)), "utm inverse")
        return lat.value, lon.value

    def longitude0(self):
        return lib().lio_utm_longitude0(self.h)

    def rtk_transform_utm(self, fix, zero_utm):
        """computeRTKTransform(projector, data, zero_utm)"""
        z, T = f64(zero_utm).reshape(3), np.zeros((4, 4))
        check(lib().lio_rtk_transform_utm(self.h, C.byref(_fix(fix)), ptr(z, C.c_double), ptr(T, C.c_double)), "rtk transform")
        return T

    def rtk_transform_origin(self, origin, fix):
        """RTKM::computeRTKTransform(origin, data)"""
        T = np.zeros((4, 4))
        check(lib().lio_rtk_transform_origin(self.h, C.byref(_fix(origin)), C.byref(_fix(fix)), ptr(T, C.c_double)), "rtk transform")
        return T


class RtkTrack:
    """lio_rtk_track: RTKM's stamp -> fix map with its interpolation, host only."""

    def __init__(self):
        self.h = lib().lio_rtk_track_create()
        if not self.h:
            raise capi.LioError("lio_rtk_track_create failed")

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_rtk_track_destroy(self.h)
        self.h = None

    __del__ = close

    def set_origin(self, fix):
        """(taken, T): the first origin wins; T is the origin's own pose"""
        T = np.zeros((4, 4))
        rc = check(lib().lio_rtk_track_set_origin(self.h, C.byref(_fix(fix)), ptr(T, C.c_double)), "track set_origin")
        return bool(rc), (T if rc else None)

    def feed(self, fix, valid=True):
        return bool(check(lib().lio_rtk_track_feed(self.h, int(bool(valid)), C.byref(_fix(fix))), "track feed"))

    def __len__(self):
        return check(lib().lio_rtk_track_size(self.h), "track size")

    def interpolate(self, stamp_us):
        """(code, T): code is one of capi.RTK_*; T is None when the track refuses"""
        T = np.zeros((4, 4))
        rc = check(lib().lio_rtk_track_interpolate(self.h, int(stamp_us), ptr(T, C.c_double)), "track interpolate")
        return rc, (T if rc in (capi.RTK_INTERPOLATED, capi.RTK_EXACT) else None)


class GnssQueue:
    """lio_gnss_queue: the pose graph's queue of fixes and its flush against the key frames, host only."""

    def __init__(self):
        self.h = lib().lio_gnss_queue_create()
        if not self.h:
            raise capi.LioError("lio_gnss_queue_create failed")
        self.last_xyz = np.zeros(3)  # gps_last_update_pose

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_gnss_queue_destroy(self.h)
        self.h = None

    __del__ = close

    def set_origin(self, fix, last_keyframe_z=None):
        z = np.zeros(3)
        check(lib().lio_gnss_queue_set_origin(self.h, C.byref(_fix(fix)), int(last_keyframe_z is not None), float(last_keyframe_z or 0.0), ptr(z, C.c_double)),
              "gnss set_origin")
        return z

    def push(self, fix):
        check(lib().lio_gnss_queue_push(self.h, C.byref(_fix(fix))), "gnss push")

    def __len__(self):
        return check(lib().lio_gnss_queue_size(self.h), "gnss size")

    def stamps(self):
        out = np.zeros(max(len(self), 1), np.uint64)
        n = check(lib().lio_gnss_queue_stamps(self.h, ptr(out, C.c_uint64), len(out)), "gnss stamps")
        return out[:n]

    def flush(self, kf_stamps, kf_has_fix):
        """the matches as dicts; kf_has_fix (uint8 array) is updated in place, self.last_xyz as well"""
        st = np.ascontiguousarray(kf_stamps, np.uint64)
        assert kf_has_fix.dtype == np.uint8 and kf_has_fix.flags.c_contiguous and len(kf_has_fix) == len(st)
        out = (capi.GnssMatch * max(len(st), 1))()
        n = check(lib().lio_gnss_queue_flush(self.h, ptr(st, C.c_uint64), ptr(kf_has_fix, C.c_uint8), len(st), ptr(self.last_xyz, C.c_double), out, len(st)),
                  "gnss flush")
        return [dict(keyframe=m.keyframe, dimension=m.dimension, first=m.first_stamp_us, second=m.second_stamp_us, xyz=np.array(m.xyz), quat=np.array(m.quat),
                     precision=m.precision) for m in out[:n]]


class ScanMerge:
    """lio_scan_merge: several lidars into one frame on the device (mergePoints + preprocessPoints of the RTKM method).  Cloud 0 is the base."""

    def __init__(self, max_clouds=16, max_points=1 << 20, device=0):
        self.h = lib().lio_scan_merge_create(device, int(max_clouds), int(max_points))
        if not self.h:
            raise capi.LioError("lio_scan_merge_create failed: " + lib().lio_last_error().decode())
        self.n = 0

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_scan_merge_destroy(self.h)
        self.h = None

    __del__ = close

    def set_transform(self, T):
        M = f64(T).reshape(4, 4)
        check(lib().lio_scan_merge_set_transform(self.h, ptr(M, C.c_double)), "scan merge set_transform")

    def run(self, clouds, stamps, headers, scan_period_us):
        """clouds: list of N_l x 4 f32; stamps: list of N_l u32; headers: u64 per cloud.  Returns (n, kept, early, late) with per-cloud counts."""
        L = len(clouds)
        pts = [f32(c).reshape(-1, 4) for c in clouds]
        sts = [np.ascontiguousarray(s, np.uint32).reshape(-1) for s in stamps]
        assert len(sts) == L and len(headers) == L and all(len(p) == len(s) for p, s in zip(pts, sts))
        pp = (C.POINTER(C.c_float) * L)(*[ptr(p, C.c_float) for p in pts])
        sp = (C.POINTER(C.c_uint32) * L)(*[ptr(s, C.c_uint32) for s in sts])
        n_l = np.array([len(p) for p in pts], np.uint32)
        hd = np.array([int(h) for h in headers], np.uint64)
        kept, early, late = np.zeros(L, np.uint32), np.zeros(L, np.uint32), np.zeros(L, np.uint32)
        n = C.c_uint64(0)
        check(lib().lio_scan_merge_run_host(self.h, L, pp, sp, ptr(n_l, C.c_uint32), ptr(hd, C.c_uint64), int(scan_period_us), ptr(kept, C.c_uint32),
                                            ptr(early, C.c_uint32), ptr(late, C.c_uint32), C.byref(n)), "scan merge run")
        self.n = int(n.value)
        return self.n, kept, early, late

    def download(self, cap=None):
        """(points, stamps) of the last run; with a cap that is too small the call's own answer -(count)"""
        cap = self.n if cap is None else int(cap)
        pts, st = np.zeros((max(cap, 1), 4), np.float32), np.zeros(max(cap, 1), np.uint32)
        m = lib().lio_scan_merge_download(self.h, ptr(pts, C.c_float), ptr(st, C.c_uint32), cap)
        if m < 0:
            if m == -self.n and self.n > cap:
                return int(m)
            check(int(m), "scan merge download")
        return pts[:m], st[:m]

    def device_view(self):
        """(points address, stamps address, n) of the last frame on the device"""
        st, n = C.POINTER(C.c_uint32)(), C.c_uint64(0)
        p = lib().lio_scan_merge_device(self.h, C.byref(st), C.byref(n))
        return p, C.cast(st, C.c_void_p).value, int(n.value)

    def last_times(self):
        """(upload_us, merge_us): device time of the last run"""
        a, b = C.c_double(0), C.c_double(0)
        check(lib().lio_scan_merge_last_times(self.h, C.byref(a), C.byref(b)), "scan merge times")
        return a.value, b.value


class InsCalib:
    """lio_calib_ins: the lidar-INS calibration (the reference's calib_ins_* chain): key scans and an odometry track in, the lidar-to-INS
    transform out.  x is the 6-vector (translation, rotation vector) of a candidate, with the time offset (s) as an optional seventh entry;
    metric 0 = global (k = 3, cap 10), 1 = local (k = 1, cap 1)."""

    GLOBAL, LOCAL, UNCAPPED = capi.CALIB_GLOBAL, capi.CALIB_LOCAL, capi.CALIB_UNCAPPED

    def __init__(self, init=None, device=0):
        self.h = lib().lio_calib_ins_create(device)
        if not self.h:
            raise capi.LioError("lio_calib_ins_create failed: " + lib().lio_last_error().decode())
        self.reset(np.eye(4) if init is None else init)

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_calib_ins_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def default_params():
        p = capi.CalibParams()
        lib().lio_calib_default_params(C.byref(p))
        return p

    def reset(self, init):
        M = f32(init).reshape(4, 4)
        check(lib().lio_calib_ins_reset(self.h, ptr(M, C.c_float)), "calib reset")

    def add_scan(self, points, stamp_us):
        """points N x (>= 3) f32; the number of points kept (about 6000 of a large scan)"""
        p = f32(points)
        p = p.reshape(-1, p.shape[-1] if p.ndim == 2 else 3)
        return check(lib().lio_calib_ins_add_scan(self.h, ptr(p, C.c_float), len(p), p.shape[1], int(stamp_us)), "calib add_scan")

    def add_odom(self, T, stamp_us):
        M = f32(T).reshape(4, 4)
        check(lib().lio_calib_ins_add_odom(self.h, ptr(M, C.c_float), int(stamp_us)), "calib add_odom")

    def counts(self):
        """(scans, odometry entries, points held)"""
        s, o, n = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        check(lib().lio_calib_ins_counts(self.h, C.byref(s), C.byref(o), C.byref(n)), "calib counts")
        return s.value, o.value, int(n.value)

    def set_transform(self, x):
        check(lib().lio_calib_ins_set_transform(self.h, ptr(f64(x).reshape(6), C.c_double)), "calib set_transform")

    def scan_matrices(self, time_offset=0.0):
        """sets the scan poses at the offset; the S x 4 x 4 f32 matrices an evaluation at the current transform uses"""
        out = np.zeros((max(self.counts()[0], 1), 4, 4), np.float32)
        check(lib().lio_calib_ins_scan_matrices(self.h, float(time_offset), ptr(out, C.c_float)), "calib scan_matrices")
        return out[: self.counts()[0]]

    def combined(self, x):
        x = f64(x).reshape(-1)
        n = self.counts()[2]
        out = np.zeros((max(n, 1), 3), np.float32)
        m = check(int(lib().lio_calib_ins_combined(self.h, ptr(x, C.c_double), len(x), ptr(out, C.c_float), n)), "calib combined")
        return out[:m]

    def error(self, x, metric):
        x, e = f64(x).reshape(-1), C.c_double(0)
        check(lib().lio_calib_ins_error(self.h, ptr(x, C.c_double), len(x), int(metric), C.byref(e)), "calib error")
        return e.value

    def error_terms(self, x, metric):
        """n x K f32: min(d2, cap) of every point's K nearest in the combined cloud, rows in combined-cloud order, ascending"""
        x = f64(x).reshape(-1)
        n, K = self.counts()[2], 2 if (int(metric) & 1) else 4
        out = np.zeros((max(n, 1), K), np.float32)
        m = check(int(lib().lio_calib_ins_error_terms(self.h, ptr(x, C.c_double), len(x), int(metric), ptr(out, C.c_float), n)), "calib error_terms")
        return out[:m]

    def calibrate(self, params=None):
        check(lib().lio_calib_ins_calibrate(self.h, C.byref(params) if params is not None else None), "calib calibrate")
        return self.result()

    def progress(self):
        """(evaluations so far, smallest cost so far, finished)"""
        n, e, f = C.c_int32(0), C.c_double(0), C.c_int32(0)
        check(lib().lio_calib_ins_progress(self.h, C.byref(n), C.byref(e), C.byref(f)), "calib progress")
        return n.value, e.value, bool(f.value)

    def result(self):
        M = np.zeros((4, 4), np.float32)
        check(lib().lio_calib_ins_result(self.h, ptr(M, C.c_float)), "calib result")
        return M

    def last_times(self):
        """(assemble_us, build_us, terms_us): device time of the last evaluation"""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        check(lib().lio_calib_ins_last_times(self.h, C.byref(a), C.byref(b), C.byref(c)), "calib times")
        return a.value, b.value, c.value


class GroundCalib:
    """lio_calib_ground: the lidar ground calibration's crop_points and fit_plane (calibration/lidar_calibration/filter.py, fit.py) on the
    device; include/lio_hip.h states every rule.  crop() or set_points() gives the handle its cloud, fit() replays fit_plane's loop over counts
    the device scored a batch of planes at a time.  The draws are this project's (`lio_ground_draw` of (seed, attempt)) or the caller's list."""

    MAX_VERTICES = capi.CALIB_GROUND_MAX_VERTICES

    def __init__(self, device=0):
        self.h = lib().lio_calib_ground_create(device)
        if not self.h:
            raise capi.LioError("lio_calib_ground_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_calib_ground_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def params(**over):
        """lio_calib_ground_params (sigma 0.05, num_iteration 100, thresh 0.9, seed 0), fields overridden by name"""
        p = capi.CalibGroundParams()
        lib().lio_calib_ground_default_params(C.byref(p))
        for k, v in over.items():
            if not hasattr(p, k):
                raise ValueError(f"lio_calib_ground_params has no field {k}")
            setattr(p, k, v)
        return p

    @staticmethod
    def _cloud(points):
        pts = f32(points)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError("points: n x (3 or more) is required")
        return pts

    def crop(self, points, polygon):
        """crop_points: the number of the n x (>= 3) f32 points that lie inside the polygon (m x 2, taken as f64); they stay on the device"""
        pts, poly = self._cloud(points), f64(np.asarray(polygon, np.float64).reshape(-1, 2))
        n = C.c_uint32(0)
        check(lib().lio_calib_ground_crop_host(self.h, ptr(pts, C.c_float), len(pts), pts.shape[1], ptr(poly, C.c_double), len(poly), C.byref(n)),
              "calib ground crop")
        return int(n.value)

    def set_points(self, points):
        """adopts n x (>= 3) f32 points as already cropped"""
        pts = self._cloud(points)
        check(lib().lio_calib_ground_set_points_host(self.h, ptr(pts, C.c_float), len(pts), pts.shape[1]), "calib ground set_points")
        return len(pts)

    def fit(self, params=None, draws=None):
        """fit_plane over the held points: (found, coef f32[4]); draws None: the seeded draws, else m x 3 indices consumed in order"""
        p = params if params is not None else self.params()
        found, co = C.c_int(0), np.zeros(4, np.float32)
        if draws is None:
            tp, nt = None, 0
        else:
            d = np.asarray(draws).reshape(-1, 3)
            if d.size and (d.min() < 0 or d.max() > 0xFFFFFFFF):
                raise ValueError("draws: indices outside 0 .. 2^32 - 1")
            t = np.ascontiguousarray(d, dtype=np.uint32)
            keep = np.zeros(3, np.uint32)  # a pointer even for an empty list: NULL means the seeded draws
            tp, nt = ptr(t if len(t) else keep, C.c_uint32), len(t)
        check(lib().lio_calib_ground_fit(self.h, C.byref(p), tp, nt, C.byref(found), ptr(co, C.c_float)), "calib ground fit")
        return bool(found.value), co

    def indices(self):
        """positions in the cropped cloud's input of the kept points, ascending"""
        n = max(-lib().lio_calib_ground_download_indices(self.h, None, 0), 0)
        out = np.zeros(n, np.uint32)
        if n > 0:
            check(int(lib().lio_calib_ground_download_indices(self.h, ptr(out, C.c_uint32), n)), "calib ground indices")
        return out

    def points(self):
        """the held points, n x 3 f32"""
        n = max(-lib().lio_calib_ground_download_points(self.h, None, 0), 0)
        out = np.zeros((n, 3), np.float32)
        if n > 0:
            check(int(lib().lio_calib_ground_download_points(self.h, ptr(out, C.c_float), n)), "calib ground points")
        return out

    def draws(self):
        """(triples n x 3 u32, colinear n bool, counts n u32, planes n x 4 f32 (NaN where colinear)) of every attempt the last fit scored"""
        n = max(-lib().lio_calib_ground_download_draws(self.h, None, None, None, None, 0), 0)
        t, col, c, pl = np.zeros((n, 3), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 4), np.float32)
        if n > 0:
            check(int(lib().lio_calib_ground_download_draws(self.h, ptr(t, C.c_uint32), ptr(col, C.c_uint32), ptr(c, C.c_uint32), ptr(pl, C.c_float), n)),
                  "calib ground draws")
        return t, col.astype(bool), c, pl

    def last_run(self):
        """dict(iterations, attempts, skipped, winner, early_exit) of fit_plane's loop as the last fit replayed it"""
        v = [C.c_int(0) for _ in range(5)]
        check(lib().lio_calib_ground_last_run(self.h, *[C.byref(x) for x in v]), "calib ground last_run")
        return dict(iterations=v[0].value, attempts=v[1].value, skipped=v[2].value, winner=v[3].value, early_exit=bool(v[4].value))

    def last_times(self):
        """(crop_us, fit_us, planes_us, score_us): device time of the last crop, of the last fit, and of its plane and score kernels"""
        v = [C.c_double(0) for _ in range(4)]
        check(lib().lio_calib_ground_last_times(self.h, *[C.byref(x) for x in v]), "calib ground times")
        return tuple(x.value for x in v)


class Boxes:
    """lio_boxes: the geometry around the reference's detection network on the device -- rotated BEV overlap, hull area, BEV IoU and GIoU3D of
    box pairs, rotated NMS with the sweep on the device, and the detector's post-process as one call; include/lio_hip.h states every rule.
    Boxes are (N, 7) f32 rows [x, y, z, dx, dy, dz, heading]; at most max_boxes on either side of a call."""

    WHAT = ("overlap", "hull", "iou_bev", "giou3d")

    def __init__(self, max_boxes=2048, device=0):
        self.h = lib().lio_boxes_create(device, max_boxes)
        if not self.h:
            raise capi.LioError("lio_boxes_create failed: " + lib().lio_last_error().decode())
        self.max_boxes = max_boxes

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_boxes_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def _rows(boxes):
        b = f32(boxes)
        if b.ndim != 2 or b.shape[1] != 7:
            raise ValueError("boxes: (N, 7) is required")
        return b

    def pairwise(self, a, b, what=WHAT):
        """dict of (len(a), len(b)) f32 matrices, one per name in `what` (of "overlap", "hull", "iou_bev", "giou3d"), from one pass"""
        a, b = self._rows(a), self._rows(b)
        for w in what:
            if w not in self.WHAT:
                raise ValueError(f"pairwise: {w!r} is not one of {self.WHAT}")
        out = {w: np.zeros((len(a), len(b)), np.float32) for w in what}
        ps = [ptr(out[w], C.c_float) if w in out else None for w in self.WHAT]
        check(lib().lio_boxes_pairwise(self.h, ptr(a, C.c_float), len(a), ptr(b, C.c_float), len(b), *ps), "boxes pairwise")
        return out

    def nms(self, boxes, scores, thresh, mode=0, max_out=None):
        """indices (int64) into `boxes` of the kept ones, best first; scores None: the boxes are already in order.  With scores the order is
        np.argsort(-scores, kind="stable").  mode capi.BOXES_NMS_AABB_GATE: the gate of the reference's nms_cpu"""
        b = self._rows(boxes)
        sc = None if scores is None else f32(np.asarray(scores).reshape(-1))
        if sc is not None and len(sc) != len(b):
            raise ValueError("nms: one score per box")
        keep = np.zeros(max(len(b), 1), np.int64)
        if max_out is not None and max_out <= 0:
            return keep[:0]
        n = check(int(lib().lio_boxes_nms(self.h, ptr(b, C.c_float), None if sc is None else ptr(sc, C.c_float), len(b), float(thresh), int(mode),
                                          0 if max_out is None else min(int(max_out), 0xFFFFFFFF), ptr(keep, C.c_int64))), "boxes nms")
        return keep[:n]

    def _post(self, fn, pb, ps, pl, n, class_thresh, nms_thresh, post_max, mode):
        ct = f32(np.asarray(class_thresh).reshape(-1))
        room = n if not post_max or post_max > n else int(post_max)
        ob, osc, ol = np.zeros((max(room, 1), 7), np.float32), np.zeros(max(room, 1), np.float32), np.zeros(max(room, 1), np.int32)
        check(lib().lio_boxes_set_gate(self.h, int(mode)), "boxes gate")
        k = check(int(fn(self.h, pb, ps, pl, n, ptr(ct, C.c_float), len(ct), float(nms_thresh), room, ptr(ob, C.c_float), ptr(osc, C.c_float),
                         ptr(ol, C.c_int32))), "boxes postprocess")
        return ob[:k], osc[:k], ol[:k]

    def postprocess(self, boxes, scores, labels, class_thresh, nms_thresh, post_max=None, mode=0):
        """(boxes (K, 7), scores (K,), labels (K,) int32) of the detector's post-process: box i passes when class_thresh[label - 1] is not
        negative and score >= it; the passing boxes through NMS in descending score (ties to the smaller index); the first post_max kept"""
        b = self._rows(boxes)
        sc, lb = f32(np.asarray(scores).reshape(-1)), np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)
        if len(sc) != len(b) or len(lb) != len(b):
            raise ValueError("postprocess: one score and one label per box")
        return self._post(lib().lio_boxes_postprocess, ptr(b, C.c_float), ptr(sc, C.c_float), ptr(lb, C.c_int32), len(b), class_thresh, nms_thresh,
                          post_max, mode)

    def postprocess_device(self, d_boxes, d_scores, d_labels, n, class_thresh, nms_thresh, post_max=None, mode=0):
        """postprocess over device addresses (ints: a tensor's data_ptr()) of n x 7 f32, n f32 and n int32 the caller has finished writing"""
        return self._post(lib().lio_boxes_postprocess_device, C.c_void_p(int(d_boxes)), C.c_void_p(int(d_scores)), C.c_void_p(int(d_labels)), int(n),
                          class_thresh, nms_thresh, post_max, mode)

    def last_indices(self):
        """positions in the caller's arrays of the boxes the last postprocess kept, in its output order (uint32)"""
        n = max(-lib().lio_boxes_last_indices(self.h, None, 0), 0)
        out = np.zeros(n, np.uint32)
        if n > 0:
            check(int(lib().lio_boxes_last_indices(self.h, ptr(out, C.c_uint32), n)), "boxes last_indices")
        return out

    def last_times(self):
        """(order_us, mask_us, sweep_us, total_us): device time of the last nms or post-process by stage; after pairwise the total alone"""
        v = [C.c_double(0) for _ in range(4)]
        check(lib().lio_boxes_last_times(self.h, *[C.byref(x) for x in v]), "boxes times")
        return tuple(x.value for x in v)


class Voxelizer:
    """lio_voxelizer: the front end of the reference's detection network on the device -- the sliding window of sweeps, the hash voxeliser and
    the mean VFE to f16; include/lio_hip.h states every rule.  Rows are (N, 5) f32 [x, y, z, intensity, time]."""

    def __init__(self, min_range, max_range, voxel_size, max_voxels, max_points_per_voxel=5, max_points=500_000, max_frame_num=1,
                 order=capi.VOXEL_ORDER_ZYX, device=0):
        p = capi.VoxelizerParams()
        for name, v in (("min_range", min_range), ("max_range", max_range), ("voxel_size", voxel_size)):
            v = [float(x) for x in np.asarray(v).reshape(-1)]
            if len(v) != 3:
                raise ValueError(f"{name}: three values are required")
            setattr(p, name, (C.c_float * 3)(*v))
        for name, v in (("max_voxels", max_voxels), ("max_points_per_voxel", max_points_per_voxel), ("max_points", max_points),
                        ("max_frame_num", max_frame_num)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name}: {v} is not an unsigned 32-bit count")
            setattr(p, name, int(v))
        p.order = int(order)
        self.params = p
        self.h = lib().lio_voxelizer_create(device, C.byref(p))
        if not self.h:
            raise capi.LioError("lio_voxelizer_create failed: " + lib().lio_last_error().decode())
        self.num_voxels = 0

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_voxelizer_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def grid_size(min_range, max_range, voxel_size):
        """[gx, gy, gz] of the reference's compute_grid_size (host only)"""
        a = [f32(np.asarray(v).reshape(-1)) for v in (min_range, max_range, voxel_size)]
        if any(len(v) != 3 for v in a):
            raise ValueError("grid_size: three values each are required")
        out = np.zeros(3, np.int32)
        check(lib().lio_voxelize_grid_size(ptr(a[0], C.c_float), ptr(a[1], C.c_float), ptr(a[2], C.c_float), ptr(out, C.c_int32)), "voxelize grid_size")
        return [int(v) for v in out]

    @staticmethod
    def _motion(motion):
        m = np.eye(4, dtype=np.float32) if motion is None else f32(np.asarray(motion).reshape(-1))
        if m.size != 16:
            raise ValueError("motion: a 4 x 4 matrix is required")
        return np.ascontiguousarray(m.reshape(-1))

    def forward(self, points, motion=None, realtime=True):
        """one frame of (N, 5) rows and the 4 x 4 motion from the previous frame to this one: the number of voxels"""
        pts = f32(points)
        if pts.ndim != 2 or pts.shape[1] != 5:
            raise ValueError("points: (N, 5) is required")
        m = self._motion(motion)
        self.num_voxels = check(int(lib().lio_voxelizer_forward(self.h, ptr(pts, C.c_float), len(pts), ptr(m, C.c_float), int(bool(realtime)))),
                                "voxelizer forward")
        return self.num_voxels

    def forward_device(self, d_points, n, motion=None, realtime=True):
        """forward over the device address (an int: a tensor's data_ptr()) of n x 5 f32 the caller has finished writing; nothing is uploaded"""
        m = self._motion(motion)
        self.num_voxels = check(int(lib().lio_voxelizer_forward_device(self.h, C.c_void_p(int(d_points)), int(n), ptr(m, C.c_float), int(bool(realtime)))),
                                "voxelizer forward_device")
        return self.num_voxels

    def output(self):
        """(features (V, 5) float16, indices (V, 4) int32, counts (V,) uint32) of the last forward"""
        v = self.num_voxels
        feat, idx, cnt = np.zeros((v, 5), np.uint16), np.zeros((v, 4), np.int32), np.zeros(v, np.uint32)
        if v > 0:
            check(int(lib().lio_voxelizer_output(self.h, ptr(feat, C.c_uint16), ptr(idx, C.c_int32), ptr(cnt, C.c_uint32), v)), "voxelizer output")
        return feat.view(np.float16), idx, cnt

    def output_device(self):
        """(address of the f16 features, address of the int32 indices, V): device memory, valid until the next forward"""
        a, b = C.c_void_p(0), C.c_void_p(0)
        v = check(int(lib().lio_voxelizer_output_device(self.h, C.byref(a), C.byref(b))), "voxelizer output_device")
        return a.value or 0, b.value or 0, v

    def window(self):
        """the window's rows (total, 5) f32, newest sweep first"""
        n = max(-int(lib().lio_voxelizer_window(self.h, None, 0)), 0)
        rows = np.zeros((n, 5), np.float32)
        if n > 0:
            check(int(lib().lio_voxelizer_window(self.h, ptr(rows, C.c_float), n)), "voxelizer window")
        return rows

    def window_counts(self):
        """rows per sweep, newest first (max_frame_num int32)"""
        out = np.zeros(self.params.max_frame_num, np.int32)
        check(int(lib().lio_voxelizer_window_counts(self.h, ptr(out, C.c_int32), len(out))), "voxelizer window_counts")
        return out

    def window_device(self):
        """(address of the window's rows on the device, rows): valid until the next forward or reset"""
        a = C.c_void_p(0)
        n = check(int(lib().lio_voxelizer_window_device(self.h, C.byref(a))), "voxelizer window_device")
        return a.value or 0, n

    def reset(self):
        check(lib().lio_voxelizer_reset(self.h), "voxelizer reset")
        self.num_voxels = 0

    def last_counts(self):
        """(real_voxels, points_in_range, points_kept) of the last forward: real_voxels above max_voxels means the cap bit"""
        v = [C.c_uint64(0) for _ in range(3)]
        check(lib().lio_voxelizer_last_counts(self.h, *[C.byref(x) for x in v]), "voxelizer counts")
        return tuple(int(x.value) for x in v)

    def last_times(self):
        """(window_us, insert_us, rank_us, slots_us, mean_us, total_us): device time of the last forward by stage"""
        v = [C.c_double(0) for _ in range(6)]
        check(lib().lio_voxelizer_last_times(self.h, *[C.byref(x) for x in v]), "voxelizer times")
        return tuple(x.value for x in v)


class ImuCalib:
    """lio_calib_imu: the lidar-IMU calibration (the reference's CalibLidarImu); include/lio_hip.h states every rule.  The host half (add_imu,
    add_frame without the flag, calibrate, the pose lists) needs no device; lidar_pose and the map update of add_frame open it on first use."""

    def __init__(self, device=0, max_scan_points=1 << 18, max_map_points=1 << 21):
        self.h = lib().lio_calib_imu_create(int(device), int(max_scan_points), int(max_map_points))
        if not self.h:
            raise capi.LioError("lio_calib_imu_create failed: " + lib().lio_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib().lio_calib_imu_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def _rows(points):
        if points is None:
            return None, 0, 4
        pts = f32(points)
        if pts.ndim != 2 or (len(pts) and pts.shape[1] < 4):
            raise ValueError("points: n x (4 or more) is required")
        return pts, len(pts), max(pts.shape[1], 4)

    def reset(self):
        check(lib().lio_calib_imu_reset(self.h), "calib imu reset")

    def add_imu(self, rows):
        """n x 7: stamp us, gyro deg/s x 3, acc g x 3"""
        r = f64(np.asarray(rows, np.float64).reshape(-1, 7))
        check(lib().lio_calib_imu_add_imu(self.h, ptr(r, C.c_double), len(r)), "calib imu add_imu")

    def add_frame(self, stamp_us, global_T, delta_T, points=None):
        pts, n, stride = self._rows(points)
        g, d = f64(np.asarray(global_T, np.float64).reshape(4, 4)), f64(np.asarray(delta_T, np.float64).reshape(4, 4))
        check(lib().lio_calib_imu_add_frame(self.h, int(stamp_us), ptr(pts, C.c_float) if n else None, n, stride, ptr(g, C.c_double), ptr(d, C.c_double)),
              "calib imu add_frame")

    def lidar_pose(self, points):
        """get_lidar_T_R: the 4 x 4 f64 pose of the frame against the local map"""
        pts, n, stride = self._rows(points)
        T = np.zeros((4, 4), np.float64)
        check(lib().lio_calib_imu_lidar_pose(self.h, ptr(pts, C.c_float) if n else None, n, stride, ptr(T, C.c_double)), "calib imu lidar_pose")
        return T

    def calibrate(self):
        R = np.zeros((3, 3), np.float64)
        check(lib().lio_calib_imu_calibrate(self.h, ptr(R, C.c_double)), "calib imu calibrate")
        return R

    def _poses(self, fn, what):
        n = self.counts()["aligned"]
        out = np.zeros((max(n, 1), 4, 4), np.float64)
        m = check(fn(self.h, ptr(out, C.c_double), len(out)), what)
        return out[:m].copy()

    def lidar_poses(self):
        return self._poses(lib().lio_calib_imu_lidar_poses, "calib imu lidar_poses")

    def imu_poses(self):
        return self._poses(lib().lio_calib_imu_imu_poses, "calib imu imu_poses")

    def counts(self):
        v = [C.c_uint32(0) for _ in range(5)]
        flag = C.c_int(0)
        check(lib().lio_calib_imu_counts(self.h, *[C.byref(x) for x in v], C.byref(flag)), "calib imu counts")
        return dict(zip(("frames", "imus", "aligned", "map_points", "target_points"), (int(x.value) for x in v)), no_rtk=bool(flag.value))

    def _download(self, fn, n, what):
        out = np.zeros((max(n, 1), 4), np.float32)
        m = check(fn(self.h, ptr(out, C.c_float), len(out)), what)
        return out[:m].copy()

    def map_download(self):
        return self._download(lib().lio_calib_imu_map_download, self.counts()["map_points"], "calib imu map_download")

    def target_download(self):
        """the matcher's target in its internal order"""
        return self._download(lib().lio_calib_imu_target_download, self.counts()["target_points"], "calib imu target_download")

    def last_times(self):
        v = [C.c_double(0) for _ in range(4)]
        check(lib().lio_calib_imu_last_times(self.h, *[C.byref(x) for x in v]), "calib imu last_times")
        return dict(zip(("stage_us", "filter_us", "align_us", "map_update_us"), (x.value for x in v)))

    def set_max_iterations(self, n):
        check(lib().lio_calib_imu_set_max_iterations(self.h, int(n)), "calib imu set_max_iterations")
