#!/usr/bin/env python3
"""Generates tests/golden/camera_path.npz: the reference's test-time camera paths (nerf/colmap_provider.py:350-397) on a fixed pose set,
computed the way the reference computes them -- scipy.spatial.transform.Rotation / Slerp in float64 -- and stored as float64.  Needs scipy
(1.15.3 when the file was written); tests/test_camera_path_cpu.py reads only the .npz, and nothing under nerf2mesh_amd/ imports scipy.

    python tests/golden/make_golden_camera_path.py

Stored:
  poses [7,4,4] f32        the set: look-at cameras at seeded positions, orthonormal in float64 and rounded once to fp32
  keys_a = [3, 0, 5], n_test_a = 4, between_a [10,4,4]
  keys_b = [6, 1],    n_test_b = 1, between_b [2,4,4]
  poses_far [2,4,4] f32    two cameras whose rotations are 179 degrees apart (about an oblique axis); between_far [7,4,4] at n_test = 6
  between_same [4,4,4]     keys [2, 2] of `poses` at n_test = 3: an identical pair
  circle [8,4,4]           camera_traj == 'circle' with n = 8 (radius 0.1, theta 80 degrees)
"""
import os

import numpy as np
from scipy.spatial.transform import Rotation, Slerp

HERE = os.path.dirname(os.path.abspath(__file__))


def look_at_set(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        c = rng.normal(size=3)
        c = c / np.linalg.norm(c) * rng.uniform(0.6, 1.4)
        z = c / np.linalg.norm(c)                              # the camera looks down -z, at the origin
        x = np.cross(rng.normal(size=3), z)
        x /= np.linalg.norm(x)
        pose = np.eye(4)
        pose[:3, :3] = np.stack([x, np.cross(z, x), z], axis=-1)
        pose[:3, 3] = c
        out.append(pose)
    return np.stack(out).astype(np.float32)


def between(poses, keys, n_test):
    """nerf/colmap_provider.py:384-395 on float64 copies of the fp32 poses."""
    poses = poses.astype(np.float64)
    out = []
    for a, b in zip(keys[:-1], keys[1:]):
        pose0, pose1 = poses[a], poses[b]
        slerp = Slerp([0, 1], Rotation.from_matrix(np.stack([pose0[:3, :3], pose1[:3, :3]])))
        for i in range(n_test + 1):
            ratio = np.sin(((i / n_test) - 0.5) * np.pi) * 0.5 + 0.5
            pose = np.eye(4)
            pose[:3, :3] = slerp(ratio).as_matrix()
            pose[:3, 3] = (1 - ratio) * pose0[:3, 3] + ratio * pose1[:3, 3]
            out.append(pose)
    return np.stack(out)


def circle(n, radius=0.1, theta_deg=80):
    """nerf/colmap_provider.py:356-376 with n frames."""
    norm = lambda v: v / (np.linalg.norm(v) + 1e-10)
    theta = np.deg2rad(theta_deg)
    out = []
    for i in range(n):
        phi = np.deg2rad(i / n * 360)
        center = np.array([radius * np.sin(theta) * np.sin(phi), radius * np.sin(theta) * np.cos(phi), radius * np.cos(theta)])
        fwd = norm(center)
        right = norm(np.cross(fwd, np.array([0, 0, 1])))
        up = norm(np.cross(right, fwd))
        pose = np.eye(4)
        pose[:3, :3] = np.stack((right, up, fwd), axis=-1)
        pose[:3, 3] = center
        out.append(pose)
    return np.stack(out)


def main():
    poses = look_at_set(7, seed=5)
    axis = np.array([0.3, -0.5, 0.81])
    far = np.stack([np.eye(4), np.eye(4)])
    far[0, :3, :3] = Rotation.from_rotvec([0.2, 0.1, -0.3]).as_matrix()
    far[1, :3, :3] = (Rotation.from_rotvec(axis / np.linalg.norm(axis) * np.deg2rad(179.0)) * Rotation.from_matrix(far[0, :3, :3])).as_matrix()
    far[0, :3, 3], far[1, :3, 3] = [0.5, -0.25, 1.0], [-0.75, 0.5, 0.125]
    far = far.astype(np.float32)
    rel = Rotation.from_matrix(far[1, :3, :3].astype(np.float64)) * Rotation.from_matrix(far[0, :3, :3].astype(np.float64)).inv()
    assert abs(np.rad2deg(rel.magnitude()) - 179.0) < 1e-3
    path = os.path.join(HERE, "camera_path.npz")
    np.savez(path, poses=poses, keys_a=np.array([3, 0, 5]), n_test_a=4, between_a=between(poses, [3, 0, 5], 4),
             keys_b=np.array([6, 1]), n_test_b=1, between_b=between(poses, [6, 1], 1),
             poses_far=far, n_test_far=6, between_far=between(far, [0, 1], 6),
             n_test_same=3, between_same=between(poses, [2, 2], 3), circle=circle(8))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
