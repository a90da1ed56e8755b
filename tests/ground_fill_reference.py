"""Test-side model of the first-keyframe ground fill (the reference's src/pcl/fill_ground_plane.cpp:21-65), written from its description: Python floats
(IEEE doubles, one operation at a time: CPython does not contract), math.sin / math.cos (the C library's, as the product's host code uses them — NOT
numpy's vectorised versions), numpy only for the final cast to float32.  The product never imports this file (tests/test_abi.py: it lives under tests/).

The RANSAC plane is ``floor_reference.ransac(cloud, 0.01)``, imported, not restated.  Eigen's Hyperplane::projection and AngleAxis::toRotationMatrix are
restated from recall, Eigen 3.3 [UPSTREAM-RECALL]; three-term sums run left to right."""
from __future__ import annotations

import math

import numpy as np

import floor_reference

RANSAC_THRESHOLD = 0.01  # ransac.setDistanceThreshold(.01), :26


def counts(params):
    """(rings, angles) of fill_cloud's two loops (:53-56) for ``params`` = (map_resolution, radius): r and angle are ACCUMULATED doubles."""
    resolution, radius = float(params[0]), float(params[1])
    return len(_rings(resolution, radius)), len(_angles(resolution, radius))


def _rings(resolution, radius):
    out, r = [], resolution
    while r <= radius:
        out.append(r)
        r += resolution
    return out


def _angles(resolution, radius):
    angle_inc = resolution / radius
    out, angle = [], 0.0
    while angle < 2 * math.pi:
        out.append(angle)
        angle += angle_inc
    return out


def ring_sample(r, normal, offset):
    """plane.projection(Vector3d(r, 0, 0)) = p - (normal . p + offset) * normal: the normal is not normalised."""
    nx, ny, nz = normal
    px, py, pz = r, 0.0, 0.0
    sd = ((nx * px + ny * py) + nz * pz) + offset
    return (px - sd * nx, py - sd * ny, pz - sd * nz)


def rotate(angle, normal, sample):
    """AngleAxis<double>(angle, normal).toRotationMatrix() * sample: the axis as it is given, about the axis through the origin."""
    nx, ny, nz = normal
    s, c = math.sin(angle), math.cos(angle)
    sin_x, sin_y, sin_z = s * nx, s * ny, s * nz
    c1 = 1.0 - c
    cos1_x, cos1_y, cos1_z = c1 * nx, c1 * ny, c1 * nz
    tmp = cos1_x * ny
    r01, r10 = tmp - sin_z, tmp + sin_z
    tmp = cos1_x * nz
    r02, r20 = tmp + sin_y, tmp - sin_y
    tmp = cos1_y * nz
    r12, r21 = tmp - sin_x, tmp + sin_x
    r00, r11, r22 = cos1_x * nx + c, cos1_y * ny + c, cos1_z * nz + c
    sx, sy, sz = sample
    return ((r00 * sx + r01 * sy) + r02 * sz, (r10 * sx + r11 * sy) + r12 * sz, (r20 * sx + r21 * sy) + r22 * sz)


def disc(normal, offset, radius, resolution):
    """The generated points alone, float32 [rings * angles, 4] (intensity 0), rings outermost."""
    normal = tuple(float(v) for v in normal)
    offset = float(offset)
    angles = _angles(float(resolution), float(radius))
    rows = []
    for r in _rings(float(resolution), float(radius)):
        sample = ring_sample(r, normal, offset)
        for angle in angles:
            x, y, z = rotate(angle, normal, sample)
            rows.append((x, y, z, 0.0))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array(rows, dtype=np.float64).reshape(-1, 4).astype(np.float32)


def fill(cloud, normal, offset, radius, resolution):
    """cloud_filled: the cloud's own points in their order, then the disc."""
    cloud = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 4))
    return np.ascontiguousarray(np.vstack([cloud, disc(normal, offset, radius, resolution)]))


def simple_plane(estimate):
    """fill_ground_plane_simple (:37-47): the third column of the rotation of the pose, offset 0."""
    e = np.asarray(estimate, dtype=np.float64).reshape(4, 4)
    return (float(e[0, 2]), float(e[1, 2]), float(e[2, 2])), 0.0


def ransac_plane(cloud):
    """fill_ground_plane_ransac (:21-35): ``floor_reference.ransac(cloud, 0.01)``; normal = (double)c[0..2], offset = (double)c[3].  Returns
    (result dict, normal or None, offset or None)."""
    r = floor_reference.ransac(cloud, RANSAC_THRESHOLD)
    if not r["has_model"]:
        return r, None, None
    c = r["coeffs"]
    return r, (float(c[0]), float(c[1]), float(c[2])), float(c[3])
