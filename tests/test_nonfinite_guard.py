"""The non-finite guard (``learner.nonfinite_guard``) on the torch path, the learner's policy and two ranks over gloo.

The torch path (runtime/train_engine.py ``_torch_guard``) folds "the gradients' squared norms sum to a finite
value" into the gate that ``GradClip.apply`` takes: the gradients of a skipped step are selected to zero and
``optimizer.step()`` still runs.  With the RL learner's Adam (betas (0, 0.99), no decay) a zero gradient leaves the
parameters bit-identical, so there the skip can be checked exactly; every comparison below is exact."""
import copy
import logging
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_dp_trainer import _free_port

CFG = {'learner': {'use_value_feature': True, 'nonfinite_guard': True}, 'model': {'enable_baselines': ['winloss']}}
NAN = float('nan')


def _rl(cfg=None, seed=0):
    from applestar_amd.rl.trainer import RLTrainer
    from applestar_amd.utils.config import deep_merge_dicts
    torch.manual_seed(seed)
    return RLTrainer(deep_merge_dicts(CFG, cfg or {}), device='cpu')


def _weights(tr):
    return {k: v.clone() for k, v in tr.model_state_dict().items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _bits(w):
    """Exact fingerprint of the fp32 tensors: the sum of each one's bit patterns."""
    return {k: int(v.contiguous().view(torch.int32).long().sum()) for k, v in w.items() if v.dtype == torch.float32}


def _poison(p, value=NAN):
    p.grad[(0,) * p.grad.dim()] = value


def _poisoned_update(tr, batch, name, value=NAN):
    """forward + backward, one bad value into the named parameter's gradient, then reduce, update, step_info."""
    tr._fwd_bwd(copy.deepcopy(batch))
    _poison(dict(tr.model.named_parameters())[name], value)
    tr._reduce()
    norm = tr._update()
    return tr.step_info({'gradient': norm})


@pytest.mark.parametrize('value', [NAN, float('inf'), 3e19])
def test_rl_torch_path_skips_and_names_the_parameter(value):
    from applestar_amd.rl.synthetic import rl_batch
    torch.set_num_threads(2)
    tr = _rl()
    assert tr.fused_opt is None and tr._gate is None         # the CPU: the torch path, no health gate of its own
    g = tr.optimizer.param_groups[0]
    assert tuple(g['betas']) == (0.0, 0.99) and g['weight_decay'] == 0.0
    batch = rl_batch(1, 2, max_entities=16, seed=3)
    info = tr.step(copy.deepcopy(batch))
    assert int(info['update_skipped']) == 0 and int(info['skipped_updates']) == 0 and int(info['nonfinite_at']) == -1
    assert tr.nonfinite_name(-1) == ''
    names = [n for n, p in tr.model.named_parameters() if p.requires_grad]
    name = names[len(names) // 2]
    w0 = _weights(tr)
    info = _poisoned_update(tr, batch, name, value)
    assert _same(w0, _weights(tr))
    assert int(info['update_skipped']) == 1 and int(info['skipped_updates']) == 1
    assert tr.nonfinite_name(int(info['nonfinite_at'])) == name
    assert int(tr._guard_status[2]) == 1 and tr._guard_counters.tolist() == [1, 1]
    if value != 3e19:                                        # (the CPU norm accumulates in double: 3e19 itself)
        assert not bool(torch.isfinite(info['gradient']))    # the log shows what the clip computed
    # two tensors at once: the first in the optimizer's order is named
    first, second = names[3], names[-2]
    tr._fwd_bwd(copy.deepcopy(batch))
    params = dict(tr.model.named_parameters())
    _poison(params[second])
    _poison(params[first], float('-inf'))
    tr._reduce()
    tr._update()
    info = tr.step_info({})
    assert _same(w0, _weights(tr))
    assert tr.nonfinite_name(int(info['nonfinite_at'])) == first
    assert int(tr._guard_status[2]) == 2 and tr._guard_counters.tolist() == [2, 2]
    # a finite step updates, ends the run of skips and keeps the total
    info = tr.step(copy.deepcopy(batch))
    w1 = _weights(tr)
    assert int(info['update_skipped']) == 0 and int(info['skipped_updates']) == 2 and int(info['nonfinite_at']) == -1
    assert tr._guard_counters.tolist() == [2, 0]
    assert not _same(w0, w1) and all(bool(torch.isfinite(v).all()) for v in w1.values() if v.is_floating_point())
    # the counters go with the optimizer and into no state dict
    assert not any('skip' in k or 'guard' in k or 'nonfinite' in k for k in tr.state_dict())
    tr.reset_optimizer()
    assert tr._guard_counters.tolist() == [0, 0]


def test_rl_without_the_guard_a_nan_reaches_the_weights():
    """What the guard is for: the same poisoned step with the guard off leaves NaN weights."""
    from applestar_amd.rl.synthetic import rl_batch
    torch.set_num_threads(2)
    tr = _rl({'learner': {'nonfinite_guard': False}})
    batch = rl_batch(1, 2, max_entities=16, seed=3)
    name = [n for n, p in tr.model.named_parameters() if p.requires_grad][5]
    tr._fwd_bwd(copy.deepcopy(batch))
    _poison(dict(tr.model.named_parameters())[name])
    tr._reduce()
    tr._update()
    assert not all(bool(torch.isfinite(v).all()) for v in _weights(tr).values() if v.is_floating_point())


def test_guard_off_adds_no_step_info_key():
    from applestar_amd.rl.synthetic import rl_batch
    from applestar_amd.rl.trainer import DEFAULT_LEARNER_CONFIG
    from applestar_amd.sl.trainer import DEFAULT_SL_CONFIG
    for d in (DEFAULT_LEARNER_CONFIG, DEFAULT_SL_CONFIG):
        assert d['learner']['nonfinite_guard'] is False and d['learner']['max_consecutive_skips'] == 10
    torch.set_num_threads(2)
    tr = _rl({'learner': {'nonfinite_guard': False}})
    assert tr.nonfinite_guard is False and tr._guard_counters is None
    info = tr.step(rl_batch(1, 2, max_entities=16, seed=3))
    assert not {'update_skipped', 'skipped_updates', 'nonfinite_at'} & set(info)
    on = _rl()
    extra = set(on.step(rl_batch(1, 2, max_entities=16, seed=3))) - set(info)
    assert extra == {'update_skipped', 'skipped_updates', 'nonfinite_at'}


def test_sl_torch_path_counts_the_skip_and_stays_finite():
    from applestar_amd.sl.trainer import SLTrainer
    from applestar_amd.rl.synthetic import sl_batch
    torch.set_num_threads(2)
    torch.manual_seed(0)
    tr = SLTrainer({'learner': {'ignore_steps': 0, 'nonfinite_guard': True, 'data': {'batch_size': 2}}})
    b = sl_batch(2, 3, max_entities=20, seed=1)
    info = tr.step(copy.deepcopy(b))
    assert int(info['update_skipped']) == 0
    name, p = [(n, q) for n, q in tr.model.named_parameters() if q.requires_grad][7]
    reduce = tr._reduce

    def poisoned_reduce():
        _poison(p)
        reduce()
    tr._reduce = poisoned_reduce
    epoch = tr.lr_scheduler.last_epoch
    info = tr.step(copy.deepcopy(b))
    tr._reduce = reduce
    assert int(info['update_skipped']) == 1 and int(info['skipped_updates']) == 1
    assert tr.nonfinite_name(int(info['nonfinite_at'])) == name
    assert tr.lr_scheduler.last_epoch == epoch + 1            # the schedule advances on a skipped step
    assert all(bool(torch.isfinite(v).all()) for v in _weights(tr).values() if v.is_floating_point())
    assert all(bool(torch.isfinite(s[k]).all()) for s in tr.optimizer.state.values() for k in ('exp_avg', 'exp_avg_sq'))
    info = tr.step(copy.deepcopy(b))
    assert int(info['update_skipped']) == 0 and int(info['skipped_updates']) == 1
    assert tr._guard_counters.tolist() == [1, 0]


# ------------------------------------------------------------------ the learner's policy
class _Records(logging.Handler):
    def __init__(self):
        super().__init__()
        self.records = []

    def emit(self, record):
        self.records.append(record)


def _learner(tmp_path, monkeypatch, skipped, limit):
    """A BaseLearner whose trainer reports ``skipped[i]`` as iteration i's ``update_skipped``."""
    from applestar_amd.learner.base_learner import BaseLearner
    from applestar_amd.learner.hooks import POSITIONS
    monkeypatch.chdir(tmp_path)

    class Stub:
        model = torch.nn.Linear(1, 1)
        optimizer = None
        total = 0

        def step(self, data):
            s = skipped[data['i']]
            self.total += s
            return {'total_loss': torch.tensor(1.0), 'update_skipped': torch.tensor(s, dtype=torch.int32),
                    'skipped_updates': torch.tensor(self.total, dtype=torch.int32),
                    'nonfinite_at': torch.tensor(4 if s else -1, dtype=torch.int32)}

        def nonfinite_name(self, index):
            return f'layer{index}.weight'

    class Learner(BaseLearner):
        def _setup_trainer(self):
            return Stub()

        def _setup_dataloader(self):
            return ({'i': i} for i in range(10 ** 6))

        def save_checkpoint(self):
            pass

    lc = {'use_cuda': False, 'log_to_stdout': False, 'nonfinite_guard': True,
          'data': {'batch_size': 2, 'trajectory_length': 4}}
    if limit is not None:
        lc['max_consecutive_skips'] = limit
    lrn = Learner({'common': {'type': 'sl'}, 'learner': lc})
    lrn.hooks = {p: [] for p in POSITIONS}
    rec = _Records()
    lrn.logger.logger.addHandler(rec)
    return lrn, rec


def test_learner_warns_and_raises_on_the_nth_consecutive_skip(tmp_path, monkeypatch):
    #          it: 1  2  3  4  5  6  7
    skipped = [1, 1, 0, 1, 1, 1, 0]
    lrn, rec = _learner(tmp_path, monkeypatch, skipped, 3)
    with pytest.raises(RuntimeError, match='3 consecutive updates skipped'):
        lrn.run(max_iterations=7)
    assert lrn.last_iter.val == 6                  # two in a row did not stop it; the third in a row did
    warns = [r.getMessage() for r in rec.records if r.levelno == logging.WARNING]
    assert len(warns) == 5
    assert 'iteration 1:' in warns[0] and 'layer4.weight' in warns[0] and '1 in a row, 1 in total' in warns[0]
    assert 'iteration 6:' in warns[-1] and '3 in a row, 5 in total' in warns[-1]
    assert lrn.log_buffer['update_skipped'] == 1.0 and lrn.log_buffer['skipped_updates'] == 5.0


def test_learner_default_limit_is_ten(tmp_path, monkeypatch):
    lrn, _ = _learner(tmp_path, monkeypatch, [1] * 12, None)
    with pytest.raises(RuntimeError, match='max_consecutive_skips = 10'):
        lrn.run(max_iterations=12)
    assert lrn.last_iter.val == 10


def test_learner_limit_zero_never_raises(tmp_path, monkeypatch):
    lrn, rec = _learner(tmp_path, monkeypatch, [1] * 15, 0)
    lrn.run(max_iterations=15)
    assert lrn.last_iter.val == 15
    assert len([r for r in rec.records if r.levelno == logging.WARNING]) == 15


# ------------------------------------------------------------------ two ranks over gloo
def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    from applestar_amd.parallel import dist as pdist
    from applestar_amd.rl.trainer import RLTrainer
    from applestar_amd.rl.synthetic import rl_batch
    pdist.init(backend='gloo')
    torch.manual_seed(rank)
    tr = RLTrainer({'learner': {'use_value_feature': True, 'bucket_mb': 4, 'nonfinite_guard': True},
                    'model': {'enable_baselines': ['winloss']}}, device='cpu')
    first = tr.step(rl_batch(1, 2, max_entities=16, seed=10 + rank))
    w0 = _weights(tr)
    # an encoder parameter: with the two-phase backward its bucket is reduced in _reduce, after the poison
    name = [n for n, p in tr.model.named_parameters() if p.requires_grad and n.startswith('encoder.')][4]
    tr._fwd_bwd(rl_batch(1, 2, max_entities=16, seed=20 + rank))
    if rank == 1:
        _poison(dict(tr.model.named_parameters())[name])
    tr._reduce()
    tr._update()
    info = tr.step_info({})
    w1 = _weights(tr)
    after = tr.step(rl_batch(1, 2, max_entities=16, seed=30 + rank))
    w2 = _weights(tr)
    q.put({'rank': rank, 'first_skipped': int(first['update_skipped']), 'skipped': int(info['update_skipped']),
           'total': int(info['skipped_updates']), 'name': tr.nonfinite_name(int(info['nonfinite_at'])),
           'want': name, 'unchanged': _same(w0, w1), 'w1': _bits(w1),
           'after_skipped': int(after['update_skipped']), 'moved': not _same(w1, w2),
           'finite': all(bool(torch.isfinite(v).all()) for v in w2.values() if v.is_floating_point()),
           'w2': _bits(w2)})
    pdist.finalize()


@pytest.mark.timeout(600)
def test_data_parallel_every_rank_skips_the_same_update():
    """World 2 (gloo): rank 1 alone has a NaN in its local gradient; the all-reduce carries it to both ranks, the
    decision follows the reduction, so both skip: their weights equal each other and those before the step."""
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in range(2)], key=lambda r: r['rank'])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r['first_skipped'] == 0 and r['skipped'] == 1 and r['total'] == 1, r['rank']
        assert r['name'] == r['want'] and r['unchanged'], r['rank']
        assert r['after_skipped'] == 0 and r['moved'] and r['finite'], r['rank']
    for stage in ('w1', 'w2'):
        assert res[0][stage] and res[0][stage] == res[1][stage], stage
