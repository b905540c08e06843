"""GPU: bench.py honours the driver's contract -- one JSON line with the required keys, the roofline
and (--full) cpu_baseline objects, whole-job throughput consistent with ms_per_step; a plain run reports the
same headline without the --full legs."""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    dump = tmp_path / 'outputs'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '1', '--full',
                          '--n_rand', '128', '--large_batch', '256', '--cpu_rays', '8', '--mip360_rays', '256',
                          '--dump-outputs', str(dump)], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1
    r = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in r, k
    assert r['n_gpus'] == 1 and r['steps'] == 4 and r['warmup'] == 1 and r['vs_baseline'] is None
    assert r['unit'] == 'rays/s' and r['higher_is_better'] is True and r['scaling'] == 'weak' and r['data'] == 'synthetic'
    assert 'workload' in r['config'] and 'model' not in r['config']
    assert abs(r['value'] - 128 / (r['ms_per_step'] * 1e-3)) <= 1e-6 * r['value']
    rf = r['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in rf, k
    assert rf['bound'] in ('hbm', 'mfma') and abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-9
    cb = r['cpu_baseline']
    assert cb['kind'] == 'port' and cb['unit'] == 'rays/s' and cb['value'] > 0 and cb['cores'] >= 1 and cb['sample']
    assert r['parity_mode']['value'] > 0 and r['large_batch']['n_rand_per_gpu'] == 256
    assert r['config5_mip360']['value'] > 0 and r['config5_mip360']['unit'] == 'rays/s'
    # --dump-outputs: the headline run's last timed step -- its per-level scalars (the loss the line reports) and parameters
    import numpy as np
    assert sorted(os.listdir(dump)) == ['last_step_scalars.npy', 'params_level0.npy', 'params_level1.npy']
    sc = np.load(dump / 'last_step_scalars.npy')
    assert sc.dtype == np.float32 and sc.shape == (2, 4)
    np.testing.assert_array_equal(sc[:, 0], np.float32(r['final_loss']))
    for m in (0, 1):
        p = np.load(dump / ('params_level%d.npy' % m))
        assert p.dtype == np.float32 and p.shape == (1202440,) and np.isfinite(p).all()
    # the same headline run again as a plain run (no --full: the other legs off, they run after it): the same line fields and
    # the same dump bit for bit, none of the --full legs; with one timed step fewer, other scalars and other parameters (the
    # dump is the LAST step's, after its update)
    short = ['--gpus', '1', '--warmup', '1', '--n_rand', '128']
    for steps in (4, 3):
        again = tmp_path / ('steps%d' % steps)
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', str(steps), '--dump-outputs', str(again)]
                             + short, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.strip().splitlines() if l.startswith('{')]
        assert len(lines) == 1
        p = json.loads(lines[0])
        for k in ('metric', 'unit', 'higher_is_better', 'dtype', 'n_gpus', 'warmup', 'scaling', 'data'):
            assert p[k] == r[k], k
        assert p['steps'] == steps and abs(p['value'] - 128 / (p['ms_per_step'] * 1e-3)) <= 1e-6 * p['value']
        assert steps != 4 or p['final_loss'] == r['final_loss']
        for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
            assert k in p['roofline'], k
        for k in ('cpu_baseline', 'parity_mode', 'parity_forward_mode', 'fp16_forward_mode', 'large_batch', 'config5_mip360',
                  'render', 'cli_loop', 'end_to_end'):
            assert k not in p, k
        assert 'vendor_gemm_same_socket' not in p['roofline']
        for f in os.listdir(dump):
            same = np.array_equal(np.load(dump / f), np.load(again / f))
            assert same == (steps == 4), (steps, f)
