"""The front end of the reference's lidar detection -- what `inference_forward` runs before its network (LidarInference::forward,
sensor_driver/inference/tensorRT/lidar_inference.cpp:81-85: the window of sweeps and the voxeliser) -- under `inference_init`'s argument names
(sensor_driver/inference/inference.py:16-25, inference.h:16-38), without the two model files.  One engine per process, as there.

Mind the reference's names: `max_points` is the points kept PER VOXEL and `max_points_use` the points the window holds
(sensor_inference/object_infer.py:19-21).  The output order is ZYX, the reference's call site."""
import numpy as np

from . import capi, lio

_engine = None


def _make(**kw):
    return lio.Voxelizer(**kw)


def voxelize_init(voxel_size, coors_range, max_points, max_voxels, max_points_use, frame_num):
    """builds the engine: coors_range is [x0, y0, z0, x1, y1, z1], voxel_size three values"""
    global _engine
    voxel_size = np.asarray(voxel_size, dtype=np.float32).reshape(-1)
    coors_range = np.asarray(coors_range, dtype=np.float32).reshape(-1)
    if voxel_size.size != 3 or coors_range.size != 6:
        raise ValueError("voxelize_init: voxel_size has three values and coors_range six")
    if _engine is not None:
        _engine.close()
        _engine = None
    _engine = _make(min_range=coors_range[:3], max_range=coors_range[3:], voxel_size=voxel_size, max_voxels=int(max_voxels),
                    max_points_per_voxel=int(max_points), max_points=int(max_points_use), max_frame_num=int(frame_num), order=capi.VOXEL_ORDER_ZYX)


def voxelize_forward(points, motion_t, realtime):
    """(voxel_features (V, 5) float16, voxel_indices (V, 4) int32) of one frame: `points` an (N, 5) array of any float dtype (ObjectInfer.process
    hands over float64), `motion_t` the 4 x 4 motion from the previous frame"""
    if _engine is None:
        raise RuntimeError("voxelize_forward: voxelize_init has not been called")
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 5:
        raise ValueError(f"voxelize_forward: points of shape (N, 5) are required, not {points.shape}")
    if points.shape[0] == 0:
        raise ValueError("voxelize_forward: at least one point is required (the reference's caller sends one zero row for an empty frame)")
    motion_t = np.asarray(motion_t)
    if motion_t.shape != (4, 4):
        raise ValueError(f"voxelize_forward: a 4 x 4 motion is required, not {motion_t.shape}")
    _engine.forward(np.ascontiguousarray(points, dtype=np.float32), np.ascontiguousarray(motion_t, dtype=np.float32), bool(realtime))
    features, indices, _ = _engine.output()
    return features, indices


def voxelize_reset():
    """inference_reset: forgets the window; 0, or -1 before voxelize_init"""
    if _engine is None:
        return -1
    _engine.reset()
    return 0
