"""Time one multi-view consistency check of depth priors (depthcons_check) at the size of the 295-frame KITTI sequence on one GPU,
and the 'mse' training step of both paths against another checkout of this package (the parent commit, built in its own tree).

    python tools/depth_consistency_bench.py [--parent /path/to/parent/checkout] [--rounds 3] [--calls 20] [--out profiles/depth_consistency_time.json]
    python tools/depth_consistency_bench.py --worker check       # the timed calls in this process

The call: 295 frames of 375 x 1242, K = 4 nearest frames, every output asked for, on the analytic plane scene of the tests at that
size (cameras 0.3 apart along x with small rotations, the plane z = 6 + 0.1 x + 0.05 y, a KITTI focal length of 721 pixels; every
pixel valid -- a dense prior, the most work the call can have).  Warm-up calls, then `calls` timed ones, each between two device
events; the median, the extremes and every time are reported.  Two windows: the library call by itself (cameras and neighbour lists
uploaded before, outputs reused: the two launches and nothing of the host) and the binding's check_async as a trainer calls it
(host validation of the cameras and lists, two small uploads, allocation, the launches).  The call is once per run: the times are
reported, not gated.  Next to them: the compulsory traffic (4 bytes read and 10 written per pixel), the ratio of the launches' time
to that traffic at the HBM rate this project uses as achievable, 6.2 TB/s, and the float64 operations the definition writes out
for this input (counted from the call's own n_valid and n_seen) over the launches' time.

The training steps: tools/depth_gnll_bench.py's workers ('mse' only), this checkout and --parent in alternating fresh processes
(the one that goes first alternates from round to round);
the parent's runs against each other are the A/A spread of the box.  Without the load-time flags a step makes exactly the calls it
made, so 'mse' of this code belongs inside that spread.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F, H, W, K = 295, 375, 1242, 4
FOCAL = 721.0
HBM_ACHIEVABLE = 6.2e12                                       # bytes / s


def plane_scene(device):
    """(depth float32 [F, H, W] on the device, cams float64 [F, 16], nbr int32 [F, K]) of the tests' analytic scene at this size"""
    import torch
    from outdoor_nerf_depth_amd import depth_consistency as DC
    rs = np.random.RandomState(0)
    c2w = np.zeros((F, 3, 4))
    for i in range(F):
        c2w[i, :, 3] = (0.3 * i, 0.05 * rs.randn(), 0.02 * i)
        a = rs.randn(3)
        a /= np.linalg.norm(a)
        th = rs.uniform(0.01, 0.06) if i % 3 else 0.0
        Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        c2w[i, :, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    Kmat = np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1.0]])
    yy, xx = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float64), torch.arange(W, device=device, dtype=torch.float64), indexing='ij')
    dc = torch.stack([(xx + 0.5 - W / 2.0) / FOCAL, (yy + 0.5 - H / 2.0) / FOCAL, torch.ones_like(xx)], -1)
    n = torch.tensor([-0.1, -0.05, 1.0], device=device, dtype=torch.float64)
    depth = torch.empty((F, H, W), dtype=torch.float32, device=device)
    for i in range(F):                                        # ray-plane intersection at the pixel centres (set-up, not timed)
        R = torch.from_numpy(c2w[i, :, :3]).to(device)
        c = torch.from_numpy(c2w[i, :, 3]).to(device)
        depth[i] = ((6.0 - n @ c) / ((dc @ R.T) @ n)).float()
    return depth, DC.pack_cams(Kmat, c2w), DC.neighbours(c2w[:, :, 3], K)


def timed(run, calls, warmup):
    """ms of `calls` calls of run(), each between two device events, after `warmup` untimed ones"""
    import torch
    for _ in range(warmup):
        res = run()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = run()
        e1.record()
        e1.synchronize()
        times.append(float(e0.elapsed_time(e1)))
    return times, res


def worker_check(calls, warmup):
    import torch
    from outdoor_nerf_depth_amd import depth_consistency as DC
    dev = torch.device('cuda:0')
    depth, cams, nbr = plane_scene(dev)
    # the launches by themselves: cameras and neighbour lists on the device already, the outputs of the first call written again, so
    # the window holds the library call (argument checks, the check launch, the rows launch) and nothing of the host side
    cams_d, nbr_d, n_views = DC.upload(cams, nbr, dev)
    prm = DC.check_params()
    first = DC.enqueue(depth, cams_d, nbr_d, n_views, prm, std=True, counts=True, rows=True)
    launches, res = timed(lambda: DC.enqueue(depth, cams_d, nbr_d, n_views, prm, std=True, counts=True, rows=True, out=first.tensors),
                          calls, warmup)
    rows = res.tensors['rows'].sum(0).cpu().numpy()
    # the binding's call as a trainer makes it: host validation of the cameras and lists, two small uploads, allocation, the launches
    out = torch.empty_like(depth)
    binding, _ = timed(lambda: DC.check_async(depth, cams, nbr, std=True, counts=True, rows=True, depth_out=out), calls, warmup)
    print(json.dumps({'launches_ms': launches, 'binding_ms': binding, 'totals': dict(zip(DC.ROW_NAMES, (int(v) for v in rows))),
                      'n_seen_total': int(res.tensors['counts'][..., 0].sum(dtype=torch.int64))}))


# float64 operations the definition writes out (an add, a multiply, a divide, a floor or a square root counted as one each; hipcc
# expands a divide into about ten instructions): to_world 24 (2 divides), to_cam 18, a projection 6 (2 divides)
OPS_PIXEL = 24 + 1                         # Pw, rel_tol * d
OPS_NEIGHBOUR = 18 + 6 + 2                 # Pj, u and v, the two floors: every listed neighbour of a valid pixel
OPS_SEEN = 2 + 24 + 18 + 6 + 2 + 3 + 1 + 2   # of a neighbour that sees the pixel: xi + .5, yi + .5, back to i, u' v', du dv, e_pix2, e, s
DIVIDES = (2, 2, 4)                        # per pixel, per listed neighbour, per seeing neighbour


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--worker', default=None, help="'check': the timed calls in this process")
    p.add_argument('--parent', default=None, help='another checkout (built) whose mse training steps alternate with this one\'s')
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--steps', type=int, default=60)
    p.add_argument('--timeout', type=int, default=300, help='seconds per worker process')
    p.add_argument('--out', default=None, help='also write the JSON result to this file')
    args = p.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    if args.worker == 'check':
        return worker_check(args.calls, args.warmup)

    def child(cmd):
        out = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=args.timeout)
        if out.returncode != 0:                               # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            sys.exit(out.returncode)
        return json.loads(out.stdout.strip().splitlines()[-1])

    got = child([os.path.abspath(__file__), '--worker', 'check', '--calls', str(args.calls), '--warmup', str(args.warmup)])
    ms, whole = got['launches_ms'], got['binding_ms']
    pixels = F * H * W
    traffic = 14 * pixels
    floor_ms = 1e3 * traffic / HBM_ACHIEVABLE
    n_valid, n_seen = got['totals']['n_valid'], got['n_seen_total']
    ops = OPS_PIXEL * n_valid + OPS_NEIGHBOUR * K * n_valid + OPS_SEEN * n_seen
    divides = DIVIDES[0] * n_valid + DIVIDES[1] * K * n_valid + DIVIDES[2] * n_seen
    med = float(np.median(ms))
    res = {'call': {'frames': F, 'height': H, 'width': W, 'views': K, 'focal': FOCAL, 'calls': args.calls, 'warmup': args.warmup,
                    'what': 'launches_ms: the library call alone (cameras and lists on the device, outputs reused); binding_ms: '
                            'depth_consistency.check_async with its host validation, uploads and allocation',
                    'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'ms': ms,
                    'binding_ms_median': float(np.median(whole)), 'binding_ms_min': min(whole), 'binding_ms_max': max(whole),
                    'binding_ms': whole, 'totals': got['totals'], 'n_seen_total': n_seen,
                    'compulsory_bytes': traffic, 'compulsory_bytes_per_pixel': {'read': 4, 'written': 10},
                    'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'ms_of_the_compulsory_traffic_at_that_rate': floor_ms,
                    'time_over_that': med / floor_ms,
                    'float64_operations_written': ops, 'of_them_divides': divides,
                    'float64_operations_written_per_s': ops / (1e-3 * med)}}
    if args.parent:
        res['mse_step'] = {'steps': args.steps, 'rounds': args.rounds, 'paths': {}}
        for path in ('mip360', 'nerfpp'):
            runs = {'parent_mse': [], 'mse': []}
            for r in range(args.rounds):                      # (who goes first alternates: a process inherits the clocks the last one left)
                for name, root in (('parent_mse', args.parent), ('mse', os.path.dirname(HERE)))[::1 if r % 2 == 0 else -1]:
                    runs[name].append(child([os.path.join(HERE, 'depth_gnll_bench.py'), '--worker', path + ':mse', '--root', root,
                                             '--steps', str(args.steps), '--warmup', '5'])['ms_per_step'])
            med = {k: float(np.median(v)) for k, v in runs.items()}
            res['mse_step']['paths'][path] = {
                'ms_per_step_runs': runs, 'ms_per_step_median': med, 'mse_minus_parent_mse_ms': med['mse'] - med['parent_mse'],
                'parent_A_A_spread_ms': max(runs['parent_mse']) - min(runs['parent_mse']),
                'mse_inside_parent_spread': bool(min(runs['parent_mse']) <= med['mse'] <= max(runs['parent_mse']))}
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
