"""bench.py driver contract on CPU: launched by torch.distributed.run with two ranks (gloo), every rank
runs the learner step, rank 0 alone prints ONE JSON line whose value is the whole-job aggregate and whose
config names the data-parallel degree (the driver's N = 1, 2, 4, 8 scaling runs use this path with RCCL)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_bench_two_ranks_prints_one_aggregate_line(tmp_path):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', '29657', os.path.join(ROOT, 'bench.py'),
           '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '1', '--unroll', '4', '--max-entities', '24']
    res = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=500)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config'):
        assert k in out, k
    assert out['n_gpus'] == 2 and out['steps'] == 2 and out['warmup'] == 1
    assert out['config']['parallelism'] == 'dp2' and out['config']['samples_per_step'] == 2 * 1 * 4
    # value = total samples over all ranks / the slowest rank's wall time
    assert abs(out['value'] - out['config']['samples_per_step'] / (out['ms_per_step'] / 1000.0)) < 0.02 * out['value']
    assert out['value'] > 0 and out['scaling'] == 'weak' and out['higher_is_better'] is True


TINY = ['--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '1', '--unroll', '4', '--max-entities', '24']
EXTRAS = ('mixed_bf16', 'sl_fp32', 'inference_p50_ms')


def _bench(tmp_path, *extra):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='')
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *TINY, *extra], cwd=str(tmp_path), env=env,
                         capture_output=True, text=True, timeout=500)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), res.stderr


@pytest.mark.timeout(600)
def test_plain_run_measures_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A plain run times --steps steps of the fp32 learner and nothing else; --dump-outputs writes the last
    step's info dict and the sampled updated weights as float32 / float64 .npy files, identical from run to run.
    That step starts from the seeded initial state: run 'c' (one step, no warm-up: the same batch) writes the same."""
    np = pytest.importorskip('numpy')
    outs = []
    for name, steps, extra in (('a', 2, ()), ('b', 2, ()), ('c', 1, ('--steps', '1', '--warmup', '0'))):
        out, err = _bench(tmp_path, *extra, '--dump-outputs', str(tmp_path / name))
        assert out['dtype'] == 'fp32' and out['steps'] == steps and out['ms_per_step'] > 0
        assert not any(k in out for k in EXTRAS), sorted(out)
        assert '[bf16]' not in err and err.count('trainer built') == 1, err[-2000:]
        # every timed step was run: one per-step figure each
        assert len([l for l in err.splitlines() if 'per-step host issue time' in l][0].split(':')[1].split()) == steps
        outs.append({f[:-4]: np.load(str(tmp_path / name / f)) for f in sorted(os.listdir(str(tmp_path / name)))})
        assert float(outs[-1]['info_total_loss']) == out['config']['final_loss']
    a, b, c = outs
    assert 'info_total_loss' in a and 'info_gradient' in a and 'params_sample' in a and a.keys() == b.keys() == c.keys()
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(a[k], c[k], equal_nan=True), k
    assert np.isfinite(a['params_sample']).all() and a['params_sample'].std() > 0


@pytest.mark.timeout(600)
def test_full_run_reports_the_other_measurements(tmp_path):
    out, err = _bench(tmp_path, '--full')
    assert out['dtype'] == 'fp32' and 'mixed_bf16' in out and 'sl_fp32' in out    # no GPU here: no inference timing
    assert out['mixed_bf16']['ms_per_step'] > 0 and out['sl_fp32']['ms_per_step'] > 0
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *TINY, '--precision', 'both'],
                         cwd=str(tmp_path), capture_output=True, text=True, timeout=100)
    assert res.returncode == 2 and '--full' in res.stderr
