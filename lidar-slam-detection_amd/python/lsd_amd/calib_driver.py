"""The reference's sensor_driver/calibration/calib_driver.py under its thirteen names, over this project's two extension modules: the six
lidar-INS functions come from `calib_driver_ext`, the seven lidar-IMU functions from `calib_imu_ext` (the reference has both halves in one
module; here `calib_driver_ext` is pinned to the INS half).  calibration/imu_calibration/calib.py and ins_calibration/calib.py of the reference
change one import line: `from lsd_amd import calib_driver as calib_driver`.  Each module is imported by the first call that
needs it, so the INS half works where the IMU module is absent and the other way round."""
import importlib

_mods = {}


def _ext(name):
    if name not in _mods:
        _mods[name] = importlib.import_module(name)
    return _mods[name]


# Lidar Ins Calibration
def calib_ins_reset(initT):
    _ext("calib_driver_ext").calib_ins_reset(initT)


def calib_ins_add_points(points, timestamp):
    _ext("calib_driver_ext").calib_ins_set_points(points, timestamp)


def calib_ins_add_odom(odom, timestamp):
    _ext("calib_driver_ext").calib_ins_set_odom(odom, timestamp)


def calib_ins_calibrate():
    _ext("calib_driver_ext").calib_ins_calibrate()


def calib_ins_get_calibration():
    return _ext("calib_driver_ext").calib_ins_get_calibration()


def calib_ins_get_calibration_transform():
    return _ext("calib_driver_ext").calib_ins_get_calibration_transform()


# Lidar Imu Calibration
def calib_imu_reset():
    _ext("calib_imu_ext").calib_imu_reset()


def calib_imu_add_points(points, timestamp, odom, pose):
    _ext("calib_imu_ext").calib_imu_set_points(points, timestamp, odom, pose)


def calib_imu_add_imu(imu_data):
    _ext("calib_imu_ext").calib_imu_set_imu(imu_data)


def calib_imu_calibrate():
    return _ext("calib_imu_ext").calib_imu_calibrate()


def calib_imu_get_lidar_poses():
    return _ext("calib_imu_ext").calib_imu_get_lidar_poses()


def calib_imu_get_imu_poses():
    return _ext("calib_imu_ext").calib_imu_get_imu_poses()


def calib_imu_get_lidar_T_R(points):
    return _ext("calib_imu_ext").calib_imu_get_lidar_T_R(points)
