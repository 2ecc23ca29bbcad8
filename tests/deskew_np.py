"""numpy restatement of the odometry frame's deskew -- what tloam_deskew_scan and the frame's k_deskew are
checked against.  Its own SE(3): the motion's log is tloam_amd.synth's closed form, the per-point exponential a vectorised
Rodrigues formula; the device uses the Sophus branches of tl_se3.hpp, so the two agree to fp64 rounding, not bit for bit.

    xi = log(motion)
    azimuth mode:  s_i = wrap_[0,2pi)(direction * (atan2(y, x) - start_azimuth)) / 2pi - ref_fraction
    timed mode:    s_i = t_i / scan_period   (a non-finite s_i or |s_i| > 2 is refused)
    p'_i = exp(s_i xi) p_i;  a non-finite return, or s_i == 0, is copied;  a motion that is bitwise the identity copies all."""
import numpy as np

from tloam_amd.synth import se3_exp_np, se3_log_np

TWO_PI = 2.0 * np.pi


def sweep_s(xyz, direction=1, start_azimuth=0.0, ref_fraction=0.0, times=None, scan_period=0.1):
    """every return's sweep time s (frame intervals, relative to the pose's instant)"""
    xyz = np.asarray(xyz, float).reshape(-1, 3)
    if times is not None:
        s = np.asarray(times, float).reshape(-1) / scan_period
        with np.errstate(invalid="ignore"):
            if not np.all(np.abs(s) <= 2.0):
                raise ValueError("a time is not finite or more than two sweeps from the pose's instant")
        return s
    with np.errstate(invalid="ignore"):
        f = float(direction) * (np.arctan2(xyz[:, 1], xyz[:, 0]) - start_azimuth)
        w = f - TWO_PI * np.floor(f / TWO_PI)
        w = np.where(w >= TWO_PI, 0.0, w)
    return w / TWO_PI - ref_fraction


def exp_act(a, p):
    """exp(a_i) p_i for twists a (N, 6) = (upsilon, omega) and points p (N, 3)"""
    u, w = a[:, :3], a[:, 3:]
    th2 = np.einsum("ij,ij->i", w, w)
    th = np.sqrt(th2)
    small = th < 1e-6
    ths = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th2 / 6.0, np.sin(ths) / ths)
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / ths ** 2)
    Cc = np.where(small, 1.0 / 6.0 - th2 / 120.0, (ths - np.sin(ths)) / ths ** 3)
    wp = np.cross(w, p)
    wu = np.cross(w, u)
    Rp = p + A[:, None] * wp + B[:, None] * np.cross(w, wp)
    Vu = u + B[:, None] * wu + Cc[:, None] * np.cross(w, wu)
    return Rp + Vu


def deskew(xyz, motion, direction=1, start_azimuth=0.0, ref_fraction=0.0, times=None, scan_period=0.1):
    """the corrected scan (N, 3); motion = the step (4x4), xi = its log"""
    xyz = np.asarray(xyz, float).reshape(-1, 3)
    motion = np.asarray(motion, float)
    s = sweep_s(xyz, direction, start_azimuth, ref_fraction, times, scan_period)
    out = xyz.copy()
    if motion.tobytes() == np.eye(4).tobytes():
        return out
    xi = se3_log_np(motion)
    sel = np.isfinite(xyz).all(axis=1) & (s != 0.0)
    out[sel] = exp_act(s[sel, None] * xi[None, :], xyz[sel])
    return out


def distort(xyz, motion, s):
    """the inverse: the points a sweep at times s would have measured, exp(s_i xi)^-1 p_i (test input)"""
    xi = se3_log_np(np.asarray(motion, float))
    out = np.asarray(xyz, float).reshape(-1, 3).copy()
    for i in range(len(out)):
        T = se3_exp_np(s[i] * xi)
        out[i] = T[:3, :3].T @ (out[i] - T[:3, 3])
    return out
