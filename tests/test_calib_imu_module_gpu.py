"""The outer boundary of the lidar-IMU calibration: the flow of the reference's ImuCalib.getPositionPoints
(calibration/imu_calibration/calib.py:85-148) restated here -- that class imports its web stack -- through lsd_amd.calib_driver: per frame
calib_imu_get_lidar_T_R, the key-frame rule (2.0 m or 5.0 in the cfg angles), calib_imu_add_points with the delta and the pose, calib_imu_add_imu;
then calib_imu_calibrate and the two pose lists.

The drive (10 frames of 16 x 120, about 1 700 points, 0.43 m and 3.1 degrees apart about all three axes, the IMU mounted at (20, -10, 35)
degrees) is chosen so that oracle/gicp.py's Vgicp converges on every frame on the CPU at these sizes (it does, to 8 mm and 6e-4 rad of the true pose).
Every pose equals the twin's (tests/calib_imu_cases.py) in f32.  The rotation from calibrate: the restatement fed with the twin's poses was
measured at 7.11e-3 rad from the true extrinsic on an MI355X (four key frames, three pairs, odometry good to a few 1e-4 rad per pair); the
product is allowed ten times that, ALLOW_TRUTH, and is held to the restatement itself within f32."""
import numpy as np
import pytest

import calib_imu_cases as CM

pytestmark = pytest.mark.gpu
ALLOW_TRUTH = 7.2e-2  # rad
STAMP0 = 1_700_000_000_000_000


def test_the_reference_flow():
    from lsd_amd import calib_driver as drv
    import calib_imu_ext as ext

    truth = CM.euler_R(*CM.GENERAL)
    drive = CM.LidarDrive(step_deg=(-1.0, 1.5, 2.5), ext_R=truth)
    frames = CM.scan_drive(n_frames=10, n_az=120, drive=drive)
    imu = CM.imu_rows(drive, -0.1, 1.1)  # the stream starts 0.1 s before the first frame
    imu[:, 0] += STAMP0
    tw, r, rule, last_pose, sent = CM.Twin(), CM.Restated(), CM.KeyFrameRule(), None, 0
    drv.calib_imu_reset()
    n_key = 0
    for i, (pts, _) in enumerate(frames):
        stamp = STAMP0 + 100_000 * i
        T = drv.calib_imu_get_lidar_T_R(pts)
        assert T.dtype == np.float32 and T.shape == (4, 4)
        Tt = tw.lidar_pose(pts)
        assert np.array_equal(T, Tt.astype(np.float32)), i
        assert i == 0 or not np.array_equal(T, np.eye(4, dtype=np.float32)), i  # every frame converges
        if rule(T):
            if last_pose is None:
                last_pose = T
            delta = np.linalg.inv(last_pose).dot(T)
            last_pose = T
            drv.calib_imu_add_points(pts, stamp, delta, T)
            tw.add_frame(pts, T.astype(np.float64))
            r.add_frame(stamp, T, delta.astype(np.float32))  # array2Eigen reads float32
            n_key += 1
        rows = imu[(imu[:, 0] > stamp - 100_000) & (imu[:, 0] <= stamp)] if i else imu[imu[:, 0] <= stamp]
        drv.calib_imu_add_imu(rows)
        r.add_imu(rows)
        sent += len(rows)
    assert n_key == 4 and ext._counts()[:2] == (4, sent) and ext._counts()[5] == 1
    R = drv.calib_imu_calibrate()
    want = r.calibrate()
    assert R.dtype == np.float32 and R.shape == (3, 3)
    e_r, e_p = CM.rot_angle(want, truth), CM.rot_angle(R.astype(np.float64), truth)
    print(f"calibrate: {len(r.aligned)} aligned frames; the restatement fed with the twin's poses is {e_r:.3e} rad from the truth, the module {e_p:.3e} rad; "
          f"largest element difference module to restatement {np.abs(R - want).max():.3e}")
    assert np.abs(R - want.astype(np.float32)).max() <= 2.0 ** -23  # one f32 step at 1
    assert e_p <= ALLOW_TRUTH
    lp, ip = drv.calib_imu_get_lidar_poses(), drv.calib_imu_get_imu_poses()
    assert len(r.aligned) == 4 and len(lp) == len(ip) == len(r.aligned) - 1
    assert np.abs(np.array(lp) - r.lidar_poses().astype(np.float32)).max() <= 2.0 ** -22  # one f32 step below 4 (m)
    assert np.abs(np.array(ip) - r.imu_poses().astype(np.float32)).max() <= 2.0 ** -22
    drv.calib_imu_reset()
    assert ext._counts() == (0, 0, 0, 0, 0, 0)
