"""Cost of the supervised loss in the SL trainer step at the bench shape (B = 6, T = 64, 512 entities, fp32, one GPU):
the fused loss (sl_loss.hip) against the torch chain.

    python tools/sl_loss_time.py [--parent-root DIR] [--repeats 3] [--steps 20] [--warmup 5] [--out FILE]

Configurations, one fresh process each, alternating (p, 0, 1, p, 0, 1, ...):
  p  the tree under ``--parent-root`` (a built checkout of the parent commit); skipped without the option
  0  this tree with ``APPLESTAR_FUSED_SL_LOSS=0`` (the torch loss)
  1  this tree with ``APPLESTAR_FUSED_SL_LOSS=1`` (the fused loss)
One JSON line per run: ``ms_per_step`` is the host clock over ``--steps`` steps between two device synchronises,
after ``--warmup`` steps on the same two batches; ``host_step_ms_median / _max`` are the host clock between the returns
of consecutive steps (no device wait), which tell one stalled step from a uniformly slow run.  The last line holds the medians, the gain and whether every fused
run is at or below the slowest torch run.  The lines also go to ``--out`` (default profiles/sl_loss_step_time.jsonl).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from applestar_amd.ops import native
    from applestar_amd.rl.synthetic import sl_batch, to_device
    from applestar_amd.sl.trainer import SLTrainer
    assert torch.cuda.is_available(), 'needs a GPU'
    native.ensure_loaded()
    torch.manual_seed(0)
    trainer = SLTrainer({'learner': {'ignore_steps': 0, 'amp_dtype': None,
                                     'data': {'batch_size': 6, 'trajectory_length': 64}}}, device='cuda')
    batches = [to_device(sl_batch(6, 64, max_entities=512, seed=i), 'cuda') for i in range(2)]
    info = None
    for i in range(args.warmup):
        info = trainer.step(dict(batches[i % 2]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks = [t0]
    for i in range(args.steps):
        info = trainer.step(dict(batches[i % 2]))
        marks.append(time.perf_counter())        # host clock at the step's return, no device wait
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    host = sorted((b - a) * 1e3 for a, b in zip(marks, marks[1:]))
    print(json.dumps({'config': args.one, 'ms_per_step': round(ms, 3), 'loss': float(info['total_loss']),
                      'fused_sl_loss': os.environ.get('APPLESTAR_FUSED_SL_LOSS', '1') != '0',
                      'host_step_ms_median': round(host[len(host) // 2], 3), 'host_step_ms_max': round(host[-1], 3)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'sl_loss_step_time.jsonl'))
    ap.add_argument('--one', choices=['p', '0', '1'], default=None, help='(internal) run one configuration')
    ap.add_argument('--root', default=HERE, help='(internal) the tree to import')
    args = ap.parse_args()
    if args.one:
        return one(args)
    assert args.repeats >= 3, 'at least three runs per configuration'
    configs = (['p'] if args.parent_root else []) + ['0', '1']
    res = {c: [] for c in configs}
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for rep in range(args.repeats):
        for c in configs:
            env = dict(os.environ)
            env.pop('APPLESTAR_FUSED_SL_LOSS', None)
            if c != 'p':
                env['APPLESTAR_FUSED_SL_LOSS'] = c
            root = os.path.abspath(args.parent_root) if c == 'p' else HERE
            cmd = [sys.executable, os.path.abspath(__file__), '--one', c, '--root', root, '--steps', str(args.steps),
                   '--warmup', str(args.warmup)]
            out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-3000:])
                raise SystemExit(f'configuration {c} failed with exit status {out.returncode}')
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            rec['repeat'] = rep
            emit(rec)
            res[c].append(rec['ms_per_step'])
    summary = {'median_ms': {c: statistics.median(v) for c, v in res.items()}}
    summary['fused_gain_ms'] = round(summary['median_ms']['0'] - summary['median_ms']['1'], 3)
    summary['every_fused_run_at_or_below_slowest_torch_run'] = max(res['1']) <= max(res['0'])
    summary['torch_spread_ms'] = round(max(res['0']) - min(res['0']), 3)
    if 'p' in res:
        summary['parent_spread_ms'] = round(max(res['p']) - min(res['p']), 3)
        summary['switch_off_minus_parent_ms'] = round(summary['median_ms']['0'] - summary['median_ms']['p'], 3)
    emit(summary)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
