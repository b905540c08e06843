"""Time the MipNeRF-360 front end on one GPU: one 375 x 1242 KITTI-sized frame through mip360.render_image (chunks of
Config.render_chunk_size = 16384 rays, the inference forward of configs/360.gin) and one mip360.sample_batch of 4096 rays
from 100 device-resident frames.  Synthetic cameras, frames and he_uniform weights; prints one JSON line.

    python tools/mip360_render_bench.py [--repeats 3] [--chunk 16384]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outdoor_nerf_depth_amd import mip360 as M                       # noqa: E402
from outdoor_nerf_depth_amd.mip360_train import he_uniform_params      # noqa: E402


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--chunk', type=int, default=16384)
    p.add_argument('--frames', type=int, default=100)
    args = p.parse_args()
    d = torch.device('cuda:0')
    H, W, F = 375, 1242, args.frames
    rs = np.random.RandomState(0)
    model = M.Mip360Model(he_uniform_params(M.mlp_shapes(M.PROP_CFG), rs), he_uniform_params(M.mlp_shapes(M.NERF_CFG), rs), d)
    p2c = np.linalg.inv(np.array([[721.5, 0, W / 2], [0, 721.5, H / 2], [0, 0, 1]]))
    c2w = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), (F, 1, 1))
    c2w[:, 2, 3] = np.linspace(0, 1, F)
    cams = torch.from_numpy(M.camera_table(p2c, c2w)).to(d)
    near, far = 0.02, 1e5
    render_s, render_all = timed(lambda: M.render_image(model, cams, 0, H, W, near, far, 1.0, args.chunk), args.repeats)
    rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=d)
    sup = torch.rand(F, H, W, device=d)
    counter = [0]

    def batch():
        counter[0] += 1
        M.sample_batch(cams, rgb, sup, 0, counter[0], 4096, near, far, depth_gt=sup)
    batch_s, batch_all = timed(batch, max(args.repeats, 20))
    chunks = -(-H * W // args.chunk)
    print(json.dumps({'frame': [H, W], 'chunk': args.chunk, 'chunks': chunks, 'render_image_s': render_s,
                      'render_image_runs_s': render_all, 'ms_per_chunk': 1e3 * render_s / chunks,
                      'sample_batch_4096_us': 1e6 * batch_s, 'estimate_render_image_s': 0.4}))


if __name__ == '__main__':
    main()
