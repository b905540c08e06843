#!/usr/bin/env python
"""Golden vectors for the MipNeRF-360 front end (tests/golden/mip360_rays.npz): camera rays of
camera_utils.pixels_to_rays and camera_utils.transform_poses_pca, computed by the upstream module itself.

    python tests/golden/make_golden_mip360_rays.py <path to nerf-methods/mipnerf360>

internal/camera_utils.py is imported with numpy standing in for jax.numpy and stub modules for the internal imports it does
not use on these paths (configs, math with math.matmul = np.matmul, stepfun, utils).  Only outputs are stored; no upstream
code is copied.  Needs upstream's non-JAX dependencies (numpy, scipy).
"""
import importlib.util
import os
import sys
import types

import numpy as np


def load_camera_utils(src):
    jax = types.ModuleType('jax')
    jax.numpy = np
    sys.modules.setdefault('jax', jax)
    sys.modules.setdefault('jax.numpy', np)
    internal = types.ModuleType('internal')
    internal.__path__ = []
    sys.modules['internal'] = internal
    for name in ('configs', 'math', 'stepfun', 'utils'):
        m = types.ModuleType('internal.' + name)
        if name == 'math':
            m.matmul = np.matmul
        if name == 'configs':
            m.Config = object                              # (type annotations only)
        if name == 'utils':
            m.Pixels = m.Rays = object
        sys.modules['internal.' + name] = m
        setattr(internal, name, m)
    spec = importlib.util.spec_from_file_location('internal.camera_utils', os.path.join(src, 'internal', 'camera_utils.py'))
    cu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cu)
    return cu


def rot(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def main(src):
    cu = load_camera_utils(src)
    out = {}
    H, W = 24, 40
    rs = np.random.RandomState(20240611)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)           # inputs representable in float32
    cams = [
        ('pinhole', cu.get_pixtocam(36.0, W, H), np.eye(3), [0.5, -0.25, 2.0], None),
        ('simple_radial', np.linalg.inv(np.array([[40., 0, 19.3], [0, 40., 12.1], [0, 0, 1]])), rot([0, 1, 0], 0.3), [0, 0, 0],
         dict(k1=-0.12, k2=0., k3=0., p1=0., p2=0.)),
        ('opencv', np.linalg.inv(np.array([[42., 0, 20.4], [0, 39., 11.7], [0, 0, 1]])), rot([1, 2, 3], 0.7), [1.5, -2.0, 0.25],
         dict(k1=-0.08, k2=0.015, k3=0., p1=0.002, p2=-0.0015)),
        ('rotated', np.linalg.inv(np.array([[30., 0, 20.], [0, 30., 12.], [0, 0, 1]])), rot([-0.4, 1, 0.2], -1.1), [-0.3, 0.8, -1.2], None),
    ]
    x, y = np.meshgrid(np.arange(W), np.arange(H), indexing='xy')
    for name, p2c, R, t, dist in cams:
        p2c = f32(p2c)
        c2w = f32(np.concatenate([R, np.asarray(t, np.float64)[:, None]], 1))
        o, d, v, r, _ = cu.pixels_to_rays(x, y, p2c, c2w, distortion_params=dist, xnp=np)
        out['cam_%s_pixtocam' % name] = p2c.astype(np.float32)
        out['cam_%s_c2w' % name] = c2w.astype(np.float32)
        out['cam_%s_dist' % name] = np.array([0.] * 7 if dist is None else
                                             [1.] + [dist.get(k, 0.) for k in ('k1', 'k2', 'k3', 'k4', 'p1', 'p2')])
        for k, a in (('origins', o), ('directions', d), ('viewdirs', v), ('radii', r)):
            out['cam_%s_%s' % (name, k)] = np.asarray(a, np.float64).reshape(H * W, -1)
    out['cam_names'] = np.array([c[0] for c in cams])
    out['hw'] = np.array([H, W])
    # transform_poses_pca on three random pose sets.  Whether its y flip is taken depends on the signs of the eigenvectors
    # LAPACK returns, not only on the poses: with this seed set 0 takes it and sets 1 and 2 do not (set 2's cameras are
    # turned upside down all the same).  tests/test_mip360_scene.py asserts both branches are covered.
    for s in range(3):
        n = 7 + 3 * s
        poses = []
        for i in range(n):
            R = rot(rs.randn(3), rs.uniform(-0.6, 0.6))
            if s == 2:
                R = R @ np.diag([1., -1., -1.])           # cameras upside down
            c = rs.randn(3) * np.array([3.0, 1.0, 0.3]) + np.array([0.5, -1.0, 2.0])
            poses.append(np.concatenate([R, c[:, None]], 1))
        poses = np.stack(poses, 0)
        pp, tf = cu.transform_poses_pca(poses)
        out['pca%d_in' % s], out['pca%d_poses' % s], out['pca%d_transform' % s] = poses, pp, tf
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mip360_rays.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
