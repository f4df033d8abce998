"""The non-finite guard of the fused clip + Adam (csrc/kernels/optim.hip ``mt_guard``, utils/fused_optim.py
``FusedClipAdam(guard=True)``) and of the trainers (``learner.nonfinite_guard``) on the GPU.

A step whose gradients hold a NaN / Inf, or a finite value whose square overflows fp32, must leave the parameters,
both Adam moments and the momentum EMA bit-identical, report where the bad value sits and count the skip - all on
the device; with finite gradients the guarded step must equal the unguarded one bit for bit.  Every comparison is
``torch.equal`` or an exact value.

The tensors are sized from the kernels' chunk length c = ``fused_adam_chunk()``: 1 element, 300 x 17, 4099 elements
whose gradient starts one element into its buffer (not 16-byte aligned: the element-wise path of the sum of
squares), exactly c, c + 1 (a one-element second chunk) and 2c + 4465 (a third chunk that ends in a one-element
tail after the float4 loop)."""
import copy

import pytest
import torch

from applestar_amd.ops import native as N

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN, INF = float('nan'), float('inf')
UNALIGNED, LAST = 2, 5                 # rows of the unaligned tensor and of the 2c + 4465 one
KINDS = [('pytorch_norm', False), ('momentum_norm', False), ('momentum_norm', True)]
KIND_IDS = ['pytorch_norm', 'momentum_norm', 'momentum_norm-segmented']
STEPS = 5


def _chunk():
    return N.ensure_loaded().fused_adam_chunk()


def _shapes():
    c = _chunk()
    return [(1,), (300, 17), (4099,), (c,), (c + 1,), (2 * c + 4465,)]


def _numels():
    return [int(torch.Size(s).numel()) for s in _shapes()]


@pytest.fixture(scope='module')
def data():
    """Initial values and STEPS sets of finite gradients for the six tensors, on the device, never modified."""
    g = torch.Generator().manual_seed(21)
    init = [torch.randn(n, generator=g).to(DEV) for n in _numels()]
    grads = [[(torch.randn(n, generator=g) * (1 + 2 * (k % 2))).to(DEV) for n in _numels()] for k in range(STEPS)]
    return init, grads


class Rig:
    """The six tensors as parameters (or as segments of ONE flat parameter), an Adam and the fused optimizer.
    ``pviews`` / ``gviews`` are flat per-row views of the parameters / of the gradient buffers the kernels read."""

    def __init__(self, data, kind, segmented=False, guard=True, device_hparams=False):
        from applestar_amd.utils.fused_optim import FusedClipAdam
        from applestar_amd.utils.grad_clip import GradClip
        init, _ = data
        n = _numels()
        segments = None
        if segmented:
            flat = torch.nn.Parameter(torch.cat(init))
            flat.grad = torch.zeros_like(flat)
            offs = [sum(n[:i]) for i in range(len(n))]
            segments = {flat: list(zip(offs, n))}
            self.params = [flat]
            self.pviews = [flat.data[o:o + k] for o, k in zip(offs, n)]
            self.gviews = [flat.grad[o:o + k] for o, k in zip(offs, n)]
        else:
            self.params = [torch.nn.Parameter(t.clone().reshape(s)) for t, s in zip(init, _shapes())]
            for i, p in enumerate(self.params):
                if i == UNALIGNED:
                    buf = torch.zeros(p.numel() + 8, device=DEV)
                    p.grad = buf[1:1 + p.numel()]
                    assert p.grad.data_ptr() % 16 == 4
                else:
                    p.grad = torch.zeros_like(p)
            self.pviews = [p.data.view(-1) for p in self.params]
            self.gviews = [p.grad.view(-1) for p in self.params]
        if kind == 'pytorch_norm':
            self.opt = torch.optim.Adam(self.params, lr=1e-3, betas=(0.5, 0.99), weight_decay=1e-4)
            self.clip = GradClip('pytorch_norm', 1.0)
            self.fused = FusedClipAdam(self.opt, 1.0, clip=self.clip, guard=guard, device_hparams=device_hparams)
        else:
            self.opt = torch.optim.Adam(self.params, lr=1e-3, weight_decay=1e-5)
            self.clip = GradClip('momentum_norm', 1.0, momentum_mode='ema')
            self.fused = FusedClipAdam(self.opt, None, clip=self.clip, segments=segments, guard=guard,
                                       device_hparams=device_hparams)
        self.grads = data[1]

    def load(self, k, poison=()):
        """Gradient set k into the buffers, then each (row, position, value) of ``poison``."""
        for v, g in zip(self.gviews, self.grads[k]):
            v.copy_(g)
        for row, pos, value in poison:
            self.gviews[row][pos] = value

    def state(self):
        """Copies of everything an update may write: parameters, both moments, the EMA and its flag."""
        out = [p.detach().clone() for p in self.params]
        for p in self.params:
            out += [self.opt.state[p][k].clone() for k in ('exp_avg', 'exp_avg_sq') if k in self.opt.state[p]]
        if self.clip.norm_mom is not None:
            out += [self.clip.norm_mom.clone(), self.clip.mom_init.clone()]
        return out

    def rows(self):
        return [v.clone() for v in self.pviews]

    def status(self):
        return self.fused.status.tolist()

    def counters(self):
        return self.fused.counters.tolist()


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _where(row, pos):
    """The (row, chunk start) that locate() must return for element ``pos`` of ``row``."""
    c = _chunk()
    return row, pos // c * c


def _positions():
    c, n = _chunk(), _numels()
    return {'first': (0, 0), 'last': (LAST, n[LAST] - 1), 'second_chunk': (LAST, c), 'unaligned': (UNALIGNED, 2050)}


def _check_located(rig, row, pos):
    skipped, first_bad, n_bad = rig.status()
    assert skipped == 1 and n_bad == 1
    got_row, off = rig.fused.locate(first_bad)
    assert (got_row, off) == _where(row, pos)
    assert off <= pos < min(off + _chunk(), _numels()[row])


@pytest.mark.parametrize('where', ['first', 'last', 'second_chunk', 'unaligned'])
@pytest.mark.parametrize('value', [NAN, INF, -INF, 3e19], ids=['nan', 'inf', '-inf', '3e19'])
@pytest.mark.parametrize('kind,segmented', KINDS, ids=KIND_IDS)
def test_poisoned_step_is_skipped_located_and_counted(data, kind, segmented, value, where):
    """Kept step, poisoned step, finite step.  3e19 is finite but its square is not (fp32 tops out at 3.4e38): the
    chunk's sum of squares is Inf, which the guard counts as non-finite on purpose."""
    row, pos = _positions()[where]
    rig = Rig(data, kind, segmented)
    rig.load(0)
    rig.fused.step()
    assert rig.status() == [0, -1, 0] and rig.counters() == [0, 0]
    snap, rows0 = rig.state(), rig.rows()
    rig.load(1, [(row, pos, value)])
    norm = rig.fused.step()
    assert _equal(rig.state(), snap)
    _check_located(rig, row, pos)
    assert rig.counters() == [1, 1]
    assert not bool(torch.isfinite(norm))                 # the norm of a skipped step is what the kernels computed
    rig.load(2)
    norm = rig.fused.step()
    rows2 = rig.rows()
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(rows0, rows2))
    assert bool(torch.isfinite(norm))
    assert rig.status() == [0, -1, 0] and rig.counters() == [1, 0]


@pytest.mark.parametrize('kind,segmented', KINDS, ids=KIND_IDS)
def test_two_poisoned_tensors_report_the_lower_chunk(data, kind, segmented):
    c = _chunk()
    rig = Rig(data, kind, segmented)
    rig.load(0)
    rig.fused.step()
    snap = rig.state()
    rig.load(1, [(4, c, INF), (1, 77, NAN)])              # the c + 1 tensor's second chunk, then an earlier tensor
    rig.fused.step()
    assert _equal(rig.state(), snap)
    skipped, first_bad, n_bad = rig.status()
    assert (skipped, n_bad) == (1, 2) and rig.fused.locate(first_bad) == (1, 0)
    rig.load(2, [(LAST, 5, NAN), (LAST, c + 5, NAN), (LAST, 2 * c + 5, NAN)])     # every chunk of one tensor
    rig.fused.step()
    assert _equal(rig.state(), snap)
    skipped, first_bad, n_bad = rig.status()
    assert (skipped, n_bad) == (1, 3) and rig.fused.locate(first_bad) == (LAST, 0)
    assert rig.counters() == [2, 2]


@pytest.mark.parametrize('kind,segmented', KINDS, ids=KIND_IDS)
def test_closed_incoming_gate(data, kind, segmented):
    """Incoming gate 0: nothing changes either way; a non-finite gradient is still reported and counted, finite
    gradients are no guarded skip and end the run of them."""
    shut, open_ = torch.zeros((), device=DEV), torch.ones((), device=DEV)
    rig = Rig(data, kind, segmented)
    rig.load(0)
    rig.fused.step(open_)
    snap, rows0 = rig.state(), rig.rows()
    row, pos = _positions()['last']
    rig.load(1, [(row, pos, NAN)])
    rig.fused.step(shut)
    assert _equal(rig.state(), snap)
    _check_located(rig, row, pos)
    assert rig.counters() == [1, 1]
    rig.load(2)
    rig.fused.step(shut)
    assert _equal(rig.state(), snap)
    assert rig.status() == [0, -1, 0] and rig.counters() == [1, 0]
    assert float(shut) == 0.0 and float(open_) == 1.0      # the caller's gate is only read
    rig.load(3)
    rig.fused.step(open_)
    assert all(not torch.equal(a, b) for a, b in zip(rows0, rig.rows()))
    assert rig.status() == [0, -1, 0] and rig.counters() == [1, 0]


@pytest.mark.parametrize('gated', [False, True], ids=['no_gate', 'open_gate'])
@pytest.mark.parametrize('kind,segmented', KINDS, ids=KIND_IDS)
def test_guard_on_equals_guard_off_bit_for_bit(data, kind, segmented, gated):
    on, off = Rig(data, kind, segmented, guard=True), Rig(data, kind, segmented, guard=False)
    assert off.fused.status is None and off.fused.counters is None
    gate = torch.ones((), device=DEV) if gated else None
    for k in range(4):
        on.load(k)
        off.load(k)
        na, nb = on.fused.step(gate), off.fused.step(gate)
        assert torch.equal(na, nb) and bool(torch.isfinite(na)), k
        assert _equal(on.state(), off.state()), k
    assert on.status() == [0, -1, 0] and on.counters() == [0, 0]


def test_binding_without_the_guard_arguments_is_the_old_call(data):
    """The three guard buffers come together or not at all."""
    rig = Rig(data, 'pytorch_norm')
    rig.load(0)
    rig.fused.step()
    f = rig.fused
    norm = torch.empty(1, device=DEV)
    args = (f._table, f._chunks, f._part, None, norm, 1.0, None, None, None, None, 1e-3, 0.5, 0.99, 1.0, 1e-8, 0.0, False)
    with pytest.raises(RuntimeError, match='guard'):
        f._C.fused_clip_adam(*args, None, f.status, None)
    before = f.counters.clone()
    f._C.fused_clip_adam(*args)
    assert torch.equal(f.counters, before) and bool(torch.isfinite(norm).all())


def test_guarded_update_in_a_graph(data):
    """One captured step() with the guard on, replayed four times; the second replay's gradients are poisoned: the
    parameters stay, the later replays update, the device counters read one skip - and the end state equals an
    eager guarded optimizer's over the same five steps."""
    cap, eager = Rig(data, 'pytorch_norm', device_hparams=True), Rig(data, 'pytorch_norm')
    row, pos = _positions()['second_chunk']
    poison = {2: [(row, pos, NAN)]}
    cap.load(0)
    cap.fused.step()                       # eager first step (creates the state)
    eager.load(0)
    eager.fused.step()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            cap.fused.step()
    torch.cuda.current_stream().wait_stream(s)
    seen = [cap.rows()]
    for k in range(1, 5):
        cap.load(k, poison.get(k, ()))
        cap.fused.prepare()
        g.replay()
        seen.append(cap.rows())
        if k == 2:
            _check_located(cap, row, pos)
            assert cap.counters() == [1, 1]
        eager.load(k, poison.get(k, ()))
        eager.fused.step()
    torch.cuda.synchronize()
    changed = [any(not torch.equal(a, b) for a, b in zip(seen[k - 1], seen[k])) for k in range(1, 5)]
    assert changed == [True, False, True, True]
    assert _equal(seen[2], seen[1])
    assert cap.status() == [0, -1, 0] and cap.counters() == [1, 0]
    assert _equal(cap.state(), eager.state()) and eager.counters() == [1, 0]
    assert all(bool(torch.isfinite(r).all()) for r in seen[4])


# ------------------------------------------------------------------ the trainers
def _trainer(prec, guard=True):
    from applestar_amd.rl.trainer import RLTrainer
    torch.manual_seed(0)
    lc = {'use_value_feature': True, 'amp_dtype': 'bfloat16' if prec == 'bf16' else None, 'learning_rate': 1e-4}
    if guard:
        lc['nonfinite_guard'] = True
    return RLTrainer({'learner': lc, 'model': {'enable_baselines': ['winloss']}}, device='cuda')


@pytest.fixture(scope='module')
def batch():
    from applestar_amd.rl.synthetic import rl_batch, to_device
    N.ensure_loaded()
    return to_device(rl_batch(2, 4, max_entities=48, seed=5), 'cuda')


@pytest.fixture(scope='module', params=['fp32', 'bf16'])
def guarded(request):
    return _trainer(request.param)


def _everything(tr):
    """Weights (the fp32 masters on the bf16 path), the bf16 compute weights and both Adam moments."""
    out = [v.clone() for v in tr.model_state_dict().values()]
    out += [p.detach().clone() for p in tr.model.parameters()]
    out += [s[k].clone() for s in tr.optimizer.state.values() for k in ('exp_avg', 'exp_avg_sq')]
    return out


def _target(tr):
    """(name, gradient buffer the optimizer reads) of the largest 2-d parameter: at least one chunk long, so the
    chunk that holds its last element starts inside it (on the bf16 path the name comes from that start)."""
    grads = tr.master._master_grad_views() if tr.master is not None else {}
    cands = [(n, p) for n, p in tr.model.named_parameters() if p.requires_grad and p.dim() == 2 and
             (tr.master is None or p in grads)]
    name, p = max(cands, key=lambda np_: np_[1].numel())
    assert p.numel() >= _chunk()
    return name, grads.get(p, p.grad)


def _poisoned_update(tr, batch):
    name, grad = _target(tr)
    tr._fwd_bwd(copy.deepcopy(batch))
    grad[-1, -1] = NAN
    tr._reduce()
    norm = tr._update()
    return name, tr.step_info({'gradient': norm})


def test_trainer_skips_names_and_recovers(guarded, batch):
    tr = guarded
    assert tr.fused_opt is not None and tr.fused_opt.guard
    info = tr.step(copy.deepcopy(batch))
    assert int(info['update_skipped']) == 0 and int(info['nonfinite_at']) == -1
    before = _everything(tr)
    total0 = int(info['skipped_updates'])
    name, info = _poisoned_update(tr, batch)
    assert _equal(_everything(tr), before)
    assert int(info['update_skipped']) == 1 and int(info['skipped_updates']) == total0 + 1
    assert tr.nonfinite_name(int(info['nonfinite_at'])) == name
    assert not bool(torch.isfinite(info['gradient']))
    info = tr.step(copy.deepcopy(batch))
    after = _everything(tr)
    assert int(info['update_skipped']) == 0 and int(info['skipped_updates']) == total0 + 1
    assert not _equal(after, before)
    assert all(bool(torch.isfinite(t).all()) for t in after if t.is_floating_point())
    tr.reset_optimizer()
    assert tr.fused_opt.counters is None or tr.fused_opt.counters.tolist() == [0, 0]


def test_graphed_trainer_step_reports_the_guard():
    """``graph_step`` with the guard: the eager first step, the capturing one and a replay all report the status
    (one static buffer on this path, handed out as a copy) and update the weights."""
    from applestar_amd.rl.synthetic import rl_batch, to_device
    from applestar_amd.rl.trainer import RLTrainer
    from applestar_amd.runtime.prefetch import entity_total_hint
    host = rl_batch(2, 4, max_entities=48, seed=5)
    batch = to_device(host, 'cuda')
    batch['entity_total'] = entity_total_hint(host)
    torch.manual_seed(0)
    tr = RLTrainer({'learner': {'use_value_feature': True, 'nonfinite_guard': True, 'graph_step': True,
                                'learning_rate': 1e-4}, 'model': {'enable_baselines': ['winloss']}}, device='cuda')
    assert tr.graph is not None and tr.fused_opt.guard
    w = [v.clone() for v in tr.model_state_dict().values()]
    for k in range(3):
        info = tr.step(copy.deepcopy(batch))
        assert [int(info[x]) for x in ('update_skipped', 'skipped_updates', 'nonfinite_at')] == [0, 0, -1], k
        assert info['update_skipped'].data_ptr() != tr.fused_opt.status.data_ptr()
        w2 = [v.clone() for v in tr.model_state_dict().values()]
        assert not _equal(w, w2) and all(bool(torch.isfinite(t).all()) for t in w2 if t.is_floating_point()), k
        w = w2
    assert tr.graph.captures == 1 and tr.graph.replays == 2 and tr.graph.eager_steps == 1


def test_trainer_without_the_guard_ends_with_nan_weights(batch):
    """What the guard is for: the same poisoned update with the guard absent."""
    tr = _trainer('fp32', guard=False)
    info = tr.step(copy.deepcopy(batch))
    assert 'update_skipped' not in info
    _poisoned_update(tr, batch)
    assert not all(bool(torch.isfinite(v).all()) for v in tr.model_state_dict().values() if v.is_floating_point())
