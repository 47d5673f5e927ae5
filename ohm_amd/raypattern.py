"""Host-side mirror (Python) of ohm::RayPattern, RayPatternConical and ClearingPattern over libohmhip.so.

  ohm::RayPattern        (ohm/RayPattern.h, .cpp)        -> RayPattern
  ohm::RayPatternConical (ohm/RayPatternConical.h, .cpp) -> RayPatternConical
  ohm::ClearingPattern   (ohm/ClearingPattern.h, .cpp)   -> ClearingPattern

A pattern is a fixed fan of rays in the sensor frame.  The host only assembles it (a few hundred points, once); it then
lives in device memory, and moving it to a pose -- buildRays, ClearingPattern.apply -- is device work: per application a
pose crosses the link, the rays never do (include/ohmhip.h, RAY PATTERNS).  The C++14 mirror of the same classes lives in
ohm_amd/host/OhmGpuMap.h.

Conventions: a rotation is a quaternion (x, y, z, w), the layout of GpuTransformSamples; a matrix is either a (4, 4) array
in the usual row, column indexing (M[r][c], translation in the last column) or 16 values already in glm's column-major
order.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from .gpumap import RayFlag

POSE_QUAT, POSE_MAT4 = 0, 1   # OHMHIP_POSE_*


def _cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def _rotate(q, v):
    """glm's quaternion * vector, q = (x, y, z, w): the operation order of include/ohmhip.h, RAY PATTERNS."""
    u = (q[0], q[1], q[2])
    uv = _cross(u, v)
    uuv = _cross(u, uv)
    return tuple(v[a] + ((uv[a] * q[3]) + uuv[a]) * 2.0 for a in range(3))


def _angle_axis(angle, axis):
    """glm::angleAxis as (x, y, z, w)."""
    s = math.sin(angle * 0.5)
    return (axis[0] * s, axis[1] * s, axis[2] * s, math.cos(angle * 0.5))


def _mat4_column_major(m):
    m = np.asarray(m, dtype=np.float64)
    if m.shape == (4, 4):
        return np.ascontiguousarray(m.T).reshape(16)
    return np.ascontiguousarray(m).reshape(16)


class RayPattern:
    """ohm::RayPattern: a set of (start, end) ray pairs relative to the sensor."""

    def __init__(self):
        self._points = []          # (x, y, z) tuples, two per ray
        self._handle = L._vp()     # the device copy, made when first needed and dropped when the pattern changes

    # -- assembling (RayPattern.cpp:24-46) ---------------------------------------------------------------------------
    def addPoints(self, points):
        """Rays from the origin to each point."""
        for p in np.asarray(points, dtype=np.float64).reshape(-1, 3):
            self.addRay((0.0, 0.0, 0.0), p)

    def addPoint(self, point):
        self.addRay((0.0, 0.0, 0.0), point)

    def addRays(self, ray_pairs):
        """(2N, 3) start / end pairs; an odd trailing point is dropped, as in the reference."""
        pairs = np.asarray(ray_pairs, dtype=np.float64).reshape(-1, 3)
        for i in range(0, pairs.shape[0] - 1, 2):
            self.addRay(pairs[i], pairs[i + 1])

    def addRay(self, ray_start, ray_end):
        self._drop_device_copy()
        self._points.append(tuple(float(v) for v in ray_start))
        self._points.append(tuple(float(v) for v in ray_end))

    def rayCount(self):
        return len(self._points) // 2

    def pointCount(self):
        return len(self._points)

    def rayPoints(self):
        """(2 * rayCount(), 3) float64: start / end pairs."""
        return np.array(self._points, dtype=np.float64).reshape(-1, 3)

    # -- device side -------------------------------------------------------------------------------------------------
    def _device_pattern(self):
        if not self._handle:
            pts = np.ascontiguousarray(self.rayPoints())
            handle = L._vp()
            L.check(L.lib.ohmhip_pattern_create(pts.ctypes.data if pts.size else None, self.rayCount(), C.byref(handle)),
                    "RayPattern: ohmhip_pattern_create")
            self._handle = handle
        return self._handle

    def _drop_device_copy(self):
        if self._handle:
            L.lib.ohmhip_pattern_destroy(self._handle)   # (waits for the device: batches in flight may read its buffers)
            self._handle = L._vp()

    def close(self):
        self._drop_device_copy()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def buildRays(self, position_or_transform, rotation=None, scaling=1.0):
        """RayPattern::buildRays, both overloads: buildRays(position, rotation, scaling=1.0) or buildRays(mat4).
        Returns the (2 * rayCount(), 3) transformed start / end pairs, computed on the device."""
        if rotation is None:
            poses, kind = _mat4_column_major(position_or_transform), POSE_MAT4
        else:
            poses = np.concatenate([np.asarray(position_or_transform, dtype=np.float64).reshape(3),
                                    np.asarray(rotation, dtype=np.float64).reshape(4)])
            kind = POSE_QUAT
        return self.buildRaysMany(poses, kind, scaling)

    def buildRaysMany(self, poses, pose_kind=POSE_QUAT, scaling=1.0):
        """Extension: the rays of K poses ((K, 7) or (K, 16)) at once, pose major: (K * 2 * rayCount(), 3)."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7 if pose_kind == POSE_QUAT else 16)
        out = np.empty((poses.shape[0] * self.pointCount(), 3), dtype=np.float64)
        L.check(L.lib.ohmhip_pattern_build_rays(self._device_pattern(), poses.ctypes.data if poses.size else None,
                                                poses.shape[0], int(pose_kind), float(scaling),
                                                out.ctypes.data if out.size else None), "RayPattern.buildRays")
        return out


class RayPatternConical(RayPattern):
    """ohm::RayPatternConical (RayPatternConical.cpp:20-75): rays inside a cone around cone_axis.  cone_angle is the
    cone's full apex angle as the reference uses it (rays deflect up to half of it), angles in radians.  The two loops
    accumulate their angles by repeated addition, as written there."""

    def __init__(self, cone_axis, cone_angle, range, angular_resolution, min_range=0.0):  # noqa: A002 (the reference's name)
        super().__init__()
        axis = [float(v) for v in cone_axis]
        inv = 1.0 / math.sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2])   # glm::normalize
        n = (axis[0] * inv, axis[1] * inv, axis[2] * inv)
        range_, min_range, step = float(range), float(min_range), float(angular_resolution)
        if not step > 0:
            raise ValueError("angular_resolution must be positive")
        self.addRay([c * min_range for c in n], [c * range_ for c in n])
        deflection_base = (n[2], n[0], n[1])
        circle_angle = 0.0
        while circle_angle < 2 * math.pi:
            deflection_axis = _rotate(_angle_axis(circle_angle, n), deflection_base)
            deflection_angle = step
            while deflection_angle <= 0.5 * cone_angle:
                ray_dir = _rotate(_angle_axis(deflection_angle, deflection_axis), n)
                self.addRay([c * min_range for c in ray_dir], [c * range_ for c in ray_dir])
                deflection_angle += step
            circle_angle += step


class ClearingPattern:
    """ohm::ClearingPattern: applies a RayPattern at a pose so that every ray lowers the first occupied voxel it meets
    and stops there -- how a map drops obstacles that have moved away.

    apply() is one call into the library (ohmhip_map_apply_pattern): rays waiting in the map's coalescing buffer are
    launched first, the batch runs with the miss value scaled by probability_scaling, and the map's miss value is what
    it was afterwards -- GpuMap.missValue() never changes.  apply_many() is an extension: K poses in one device batch,
    with the result of K apply() calls."""

    kDefaultRayFlags = (RayFlag.kRfEndPointAsFree | RayFlag.kRfStopOnFirstOccupied | RayFlag.kRfExcludeFree |
                        RayFlag.kRfExcludeUnobserved)   # ohm/ClearingPattern.h:44-45

    def __init__(self, pattern, take_ownership=False):
        self._pattern = pattern
        self._owns = bool(take_ownership)
        self._ray_flags = int(self.kDefaultRayFlags)
        self._have_last = False

    def pattern(self):
        return self._pattern

    def hasPatternOwnership(self):
        return self._owns

    def rayFlags(self):
        return self._ray_flags

    def setRayFlags(self, ray_flags):
        """ClearingPattern.cpp:40-44: kRfReverseWalk is never set for a clearing pattern."""
        self._ray_flags = int(ray_flags) & ~int(RayFlag.kRfReverseWalk)

    def apply(self, gpu_map, position_or_transform, rotation=None, probability_scaling=1.0):
        """apply(gpu_map, position, rotation, probability_scaling=1.0) or apply(gpu_map, mat4, probability_scaling=...).
        Returns the number of points integrated (2 per ray the map's ray filter passed)."""
        if rotation is None:
            return self.apply_many(gpu_map, _mat4_column_major(position_or_transform), probability_scaling, POSE_MAT4)
        pose = np.concatenate([np.asarray(position_or_transform, dtype=np.float64).reshape(3),
                               np.asarray(rotation, dtype=np.float64).reshape(4)])
        return self.apply_many(gpu_map, pose, probability_scaling, POSE_QUAT)

    def apply_many(self, gpu_map, poses, probability_scaling=1.0, pose_kind=POSE_QUAT):
        """The pattern at each of K poses ((K, 7): translation xyz, rotation xyzw; or (K, 16) column-major matrices with
        pose_kind=POSE_MAT4), in one device batch.  The batch replays its rays in order, so the map is the one K apply()
        calls leave: a later pose's rays see what an earlier pose cleared."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7 if pose_kind == POSE_QUAT else 16)
        gpu_map._push_config_if_changed()   # the host map's values, as before every batch
        done = C.c_size_t(0)
        status = L.lib.ohmhip_map_apply_pattern(gpu_map._handle, self._pattern._device_pattern(),
                                                poses.ctypes.data if poses.size else None, poses.shape[0],
                                                int(pose_kind), 1.0, float(probability_scaling), self._ray_flags,
                                                C.byref(done))
        L.check(status, "ClearingPattern.apply")
        self._have_last = poses.shape[0] > 0 and self._pattern.rayCount() > 0
        return int(done.value)

    def lastRaySet(self):
        """The rays of the last apply() / apply_many() (or of a buildRays() on the pattern since): (elements, 3) float64
        start / end pairs, read back from the device buffer the batch was given."""
        if not self._have_last:
            return np.empty((0, 3), dtype=np.float64)
        n = C.c_size_t(0)
        handle = self._pattern._device_pattern()
        L.check(L.lib.ohmhip_pattern_last_rays(handle, None, C.byref(n)), "ClearingPattern.lastRaySet")
        out = np.empty((int(n.value), 3), dtype=np.float64)
        if out.size:
            L.check(L.lib.ohmhip_pattern_last_rays(handle, out.ctypes.data, C.byref(n)), "ClearingPattern.lastRaySet")
        return out
