"""The defined arithmetic of ohm::RayPattern / RayPatternConical (ohm/RayPattern.cpp:58-84, ohm/RayPatternConical.cpp:20-75)
as a CPU model: plain Python floats (IEEE binary64), one rounding per operation, in the order written here.  The device
kernel k_pattern_rays (ohm_amd/csrc/pattern_kernels.h) and both host mirrors are held to this model bit for bit.

The operation order of the two glm products (quaternion * vector, mat4 * vec4) is restated from glm's sources as they are
published; glm itself is not available to confirm it against, so the order below is the DEFINITION.

Test infrastructure only: nothing under ohm_amd/ imports this.
"""
import math

import numpy as np

POSE_QUAT, POSE_MAT4 = 0, 1   # ohmhip_pattern_build_rays / ohmhip_map_apply_pattern pose_kind
POSE_DOUBLES = {POSE_QUAT: 7, POSE_MAT4: 16}


def cross(a, b):
    """glm::cross: (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y)"""
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def quat_rotate(q, v):
    """glm: operator*(qua, vec3).  q = (x, y, z, w).  v + ((uv * q.w) + uuv) * 2 with uv = cross(u, v), uuv = cross(u, uv)."""
    u = (q[0], q[1], q[2])
    uv = cross(u, v)
    uuv = cross(u, uv)
    w = q[3]
    return tuple(v[a] + ((uv[a] * w) + uuv[a]) * 2.0 for a in range(3))


def transform_point_quat(pose, sample, scaling=1.0):
    """rotation * (scaling * sample) + position (RayPattern.cpp:65).  pose: translation xyz, rotation x, y, z, w."""
    s = (scaling * sample[0], scaling * sample[1], scaling * sample[2])
    r = quat_rotate(pose[3:7], s)
    return (r[0] + pose[0], r[1] + pose[1], r[2] + pose[2])


def transform_point_mat4(m, sample, scaling=1.0):
    """dvec3(pattern_transform * dvec4(sample, 1)) (RayPattern.cpp:79).  m: 16 doubles, column major (m[c][r] = m[4c + r]);
    per row r: (m[0][r]*x + m[1][r]*y) + (m[2][r]*z + m[3][r]), with (x, y, z) = scaling * sample (the reference's matrix
    overload has no scaling argument: scaling 1 is that overload, the product by 1.0 being exact)."""
    x, y, z = scaling * sample[0], scaling * sample[1], scaling * sample[2]
    return tuple((m[0 + r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r]) for r in range(3))


def build_rays(ray_points, poses, pose_kind=POSE_QUAT, scaling=1.0):
    """The rays of `poses` applied to the pattern, pose major in pattern order: (poses * points, 3) float64.
    ray_points: (2R, 3) start / end pairs; poses: (K, 7) or (K, 16)."""
    pts = np.asarray(ray_points, dtype=np.float64).reshape(-1, 3)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, POSE_DOUBLES[pose_kind])
    out = np.empty((poses.shape[0] * pts.shape[0], 3), dtype=np.float64)
    scaling = float(scaling)
    at = 0
    for pose in poses:
        p = [float(v) for v in pose]
        for pt in pts:
            s = (float(pt[0]), float(pt[1]), float(pt[2]))
            out[at] = transform_point_quat(p, s, scaling) if pose_kind == POSE_QUAT else \
                transform_point_mat4(p, s, scaling)
            at += 1
    return out


def angle_axis(angle, axis):
    """glm::angleAxis: (w = cos(a/2), xyz = axis * sin(a/2)); returned as (x, y, z, w).  The axis is NOT normalised."""
    s = math.sin(angle * 0.5)
    return (axis[0] * s, axis[1] * s, axis[2] * s, math.cos(angle * 0.5))


def normalize(v):
    """glm::normalize: v * (1 / sqrt(dot(v, v))), dot = (x*x + y*y) + z*z."""
    inv = 1.0 / math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return (v[0] * inv, v[1] * inv, v[2] * inv)


def conical_ray_points(cone_axis, cone_angle, range_, angular_resolution, min_range=0.0):
    """RayPatternConical's constructor (RayPatternConical.cpp:20-75): (2R, 3) start / end pairs.  Both loop counters are
    accumulated by repeated addition, as written there."""
    n = normalize([float(v) for v in cone_axis])
    pts = [tuple(c * min_range for c in n), tuple(c * range_ for c in n)]
    deflection_base = (n[2], n[0], n[1])
    circle_angle = 0.0
    while circle_angle < 2 * math.pi:
        deflection_axis = quat_rotate(angle_axis(circle_angle, n), deflection_base)
        deflection_angle = angular_resolution
        while deflection_angle <= 0.5 * cone_angle:
            ray_dir = quat_rotate(angle_axis(deflection_angle, deflection_axis), n)
            pts.append(tuple(c * min_range for c in ray_dir))
            pts.append(tuple(c * range_ for c in ray_dir))
            deflection_angle += angular_resolution
        circle_angle += angular_resolution
    return np.array(pts, dtype=np.float64).reshape(-1, 3)


def spherical_image(ray_points, angular_resolution):
    """The quantisation of tests/ohmtest/RayPatternTests.cpp:112-150: ray ends rasterised into an azimuth x elevation
    image, 255 where a ray ends.  Returns (image uint8 flat, width, height)."""
    height = int(math.ceil(math.pi / angular_resolution))
    width = int(math.ceil(2.0 * math.pi / angular_resolution))
    image = np.zeros(width * height, dtype=np.uint8)
    ends = np.asarray(ray_points, dtype=np.float64).reshape(-1, 3)[1::2]
    for end in ends:
        x, y, z = (float(c) for c in end)
        scale_2d = math.sqrt(x * x + y * y)
        f = 1.0 / scale_2d if scale_2d else 0.0
        azimuth = math.atan2(y * f, x * f)
        elevation = math.atan2(z, scale_2d)
        if azimuth < 0:
            azimuth += 2.0 * math.pi
        ab = int(azimuth / angular_resolution)
        eb = int((elevation + 0.5 * math.pi) / angular_resolution)
        assert 0 <= ab < width and 0 <= eb < height, (ab, eb)
        image[ab + eb * width] = 255
    return image, width, height


def filter_good_count(rays, filter_range=1e10):
    """Rays the map's default filter accepts (ohm/RayFilter.cpp goodRay with a range: finite ends, squared length
    (rx*rx + ry*ry) + rz*rz <= range^2)."""
    r = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    with np.errstate(invalid="ignore", over="ignore"):
        d = r[:, 3:] - r[:, :3]
        len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        good = np.isfinite(r).all(axis=1) & (len2 <= filter_range * filter_range)
    return int(good.sum())
