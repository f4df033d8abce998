"""The fused supervised loss on the GPU (csrc/kernels/sl_loss.hip): the per-row cross entropy and its backward, the
selected-units form, the one-workgroup tail, ``SupervisedLoss`` with the switch on against off, one trainer step.

Error rule for the losses (the project's convention for a kernel that replaces a torch chain): the kernel's largest
error against float64 is at most 4x the largest error of the torch fp32 chain on the same values against the same
float64, with a floor of one fp32 ulp of the largest value.  Gradients: 1e-4 (fp32) / 2e-2 (bf16) of
max(1, |reference|max), the bounds of ``test_head_stats_matches_reference``."""
import numpy as np
import pytest
import torch

from applestar_amd import ops
from applestar_amd.ops import native as N
from applestar_amd.ops import reference as R
from applestar_amd.sl import loss as L
from applestar_amd.sl.loss import SupervisedLoss, _ce

pytestmark = pytest.mark.gpu

DEV = 'cuda'
HEADS = SupervisedLoss.HEADS
FLAT = R.SL_FLAT_HEADS


@pytest.fixture(scope='module', autouse=True)
def _load():
    N.ensure_loaded()


def _ulp(v: float) -> float:
    return float(np.spacing(np.float32(abs(v))))


def _check_loss_rule(got, torch32, want64, what=''):
    """got / torch32: fp32 results of the kernel and of the torch chain; want64: float64 on the same values."""
    ek = float((got.double().cpu() - want64).abs().max())
    et = float((torch32.double().cpu() - want64).abs().max())
    bound = max(4 * et, _ulp(float(want64.abs().max())))
    print(f'{what} kernel err {ek:.3e} torch err {et:.3e} bound {bound:.3e}')
    assert ek <= bound, (what, ek, et, bound)


def _grad_tol(dtype):
    return 2e-2 if dtype == torch.bfloat16 else 1e-4


def _tied_columns(C):
    """Two columns of the unmasked lower half held by different lanes and, for a workgroup row, different waves."""
    if C == 2:
        return 0, 1
    if C > 4096:
        return 5, 130                  # threads 5 and 130 of 256: waves 0 and 2
    return 3, (72 if C // 2 > 72 else 20)


def _ce_inputs(R_, C, dtype):
    """3 randn, the upper half of the columns at -1e9 when C > 4, one fully masked row (R > 3), one planted tie.
    Every other row's maximum is unique in the storage dtype (checked here; the next seed otherwise), so that the
    argmax compares exactly.  Returns CPU tensors: values in the storage dtype, labels, tied row, masked row."""
    tied = 1 if R_ > 1 else 0
    full = 3 if R_ > 3 else None
    c0, c1 = _tied_columns(C)
    for seed in range(100):
        g = torch.Generator().manual_seed(1000 * seed + 7 * R_ + C)
        x = (3 * torch.randn(R_, C, generator=g)).to(dtype)
        if C > 4:
            x[:, C // 2:] = -1e9
        if full is not None:
            x[full] = -1e9
        top = (x[tied].float().max() + 1.0).to(dtype)
        x[tied, c0] = top
        x[tied, c1] = top
        rows = [r for r in range(R_) if r != tied and r != full]
        xs = x[rows].float()
        if rows and not bool(((xs == xs.max(-1, keepdim=True).values).sum(-1) == 1).all()):
            continue
        lab = torch.randint(0, max(1, C // 2), (R_,), generator=g)
        return x, lab, tied, full
    raise AssertionError('no seed gives unique maxima')


CE_SHAPES = [(r, c) for r in (1, 5, 37) for c in (2, 64, 65, 327, 4096, 4097)] + [(5, 24320)]


@pytest.mark.parametrize('with_row_on', [False, True])
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('R_,C', CE_SHAPES)
def test_sl_head_ce_matches_float64(R_, C, dtype, eps, with_row_on):
    x, lab, tied, full = _ce_inputs(R_, C, dtype)
    on = None
    if with_row_on:
        on = torch.ones(R_, dtype=torch.bool)
        on[R_ // 2] = False                      # R = 1: the only row is off
        if R_ > 4:
            on[4] = False
    want, want_amax = R.sl_head_ce(x.double(), lab, eps, row_on=on)
    xg = x.to(DEV)
    if on is not None:
        xg[~on.to(DEV)] = float('nan')           # switched-off rows are not read
    lg = xg.clone().requires_grad_(True)
    got, amax = ops.sl_head_ce(lg, lab.to(DEV), eps, row_on=None if on is None else on.to(DEV))
    assert got.dtype == torch.float32 and amax.dtype == torch.int64 and got.shape == (R_,)
    assert torch.equal(amax.cpu(), want_amax)
    c0, _ = _tied_columns(C)
    if on is None or bool(on[tied]):
        assert int(amax[tied]) == c0
    if full is not None and (on is None or bool(on[full])):
        assert int(amax[full]) == 0
        assert abs(float(got[full].detach()) - float(np.log(C))) <= 2 * _ulp(float(np.log(C)))
    # the torch fp32 chain on the same values (zeros in the switched-off rows, their loss masked)
    xt = torch.where(on.to(DEV)[:, None], x.to(DEV), torch.zeros((), dtype=dtype, device=DEV)) if on is not None \
        else x.to(DEV)
    lt = xt.clone().requires_grad_(True)
    chain = _ce(lt, lab.to(DEV), eps)
    if on is not None:
        chain = chain * on.to(DEV)
        assert torch.all(got[~on.to(DEV)] == 0) and torch.all(amax[~on.to(DEV)] == -1)
    assert bool(torch.isfinite(got).all())
    _check_loss_rule(got.detach(), chain.detach(), want, f'ce R={R_} C={C} {dtype} eps={eps}')
    g = torch.randn(R_, generator=torch.Generator().manual_seed(5)).to(DEV)
    if R_ > 2:
        g[2] = 0.0
    got.backward(g)
    chain.backward(g)
    assert lg.grad.dtype == dtype
    ref_grad = lt.grad.float()
    err = float((lg.grad.float() - ref_grad).abs().max())
    assert err <= _grad_tol(dtype) * max(1.0, float(ref_grad.abs().max())), err
    if R_ > 2:
        assert torch.all(lg.grad[2] == 0)
    if on is not None:
        assert torch.all(lg.grad[~on.to(DEV)] == 0)


# ------------------------------------------------------------------------------------------ selected-units form
def _su_inputs(b, S, n, dtype):
    g = torch.Generator().manual_seed(b * 100 + S)
    if b == 5:
        lengths = torch.tensor([0, 1, 3, S, 2])
        on = torch.tensor([True, True, False, True, True])
        long_row = 3
    else:
        lengths = torch.tensor([3, S, 2])
        on = torch.tensor([False, True, True])
        long_row = 1
    entity_num = torch.full((b,), n - 1)
    labels = torch.randint(0, n - 1, (b, S), generator=g)
    labels[long_row, :S - 1] = torch.randperm(n - 1, generator=g)[:S - 1] if n - 1 >= S - 1 else \
        torch.randint(0, n - 1, (S - 1,), generator=g)
    labels[long_row, 3] = labels[long_row, 1]                      # one unit labelled twice
    for i in range(b):
        if lengths[i] > 0:
            labels[i, lengths[i] - 1] = entity_num[i]                 # the end flag at len - 1
    logits = (2 * torch.randn(b, S, n, generator=g)).to(dtype)
    return logits, labels, lengths, on


@pytest.mark.parametrize('su_mask', [True, False])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('b,S,n', [(5, 64, 513), (3, 7, 13)])
def test_sl_head_ce_selected_units_form(b, S, n, dtype, su_mask):
    logits, labels, lengths, on = _su_inputs(b, S, n, dtype)
    want, _ = R.sl_head_ce(logits.double(), labels, 0.0, su=(lengths, on), su_mask=su_mask)
    l32 = logits.float().clone().requires_grad_(True)
    cpu32, _ = R.sl_head_ce(l32, labels, 0.0, su=(lengths, on), su_mask=su_mask)
    row_on = (torch.arange(S)[None] < lengths[:, None]) & on[:, None]
    dev = lambda t: t.to(DEV)  # noqa: E731
    outs = []
    for poison in (False, True):
        xg = dev(logits).clone()
        if poison:
            xg[~dev(row_on)] = float('nan')
        lg = xg.requires_grad_(True)
        got, amax = ops.sl_head_ce(lg, dev(labels), 0.0, su=(dev(lengths), dev(on)), su_mask=su_mask)
        g = torch.randn(b, S, generator=torch.Generator().manual_seed(9))
        got.backward(dev(g))
        outs.append((got.detach().cpu(), amax.cpu(), lg.grad.cpu()))
    (got, amax, grad), (got_p, amax_p, grad_p) = outs
    assert bool(torch.isfinite(got_p).all()) and bool(torch.isfinite(grad_p.float()).all())
    assert torch.equal(got, got_p) and torch.equal(amax, amax_p) and torch.equal(grad, grad_p)
    assert got.shape == (b, S) and torch.all(got[~row_on] == 0) and torch.all(amax[~row_on] == -1)
    _check_loss_rule(got, cpu32.detach(), want, f'su b={b} S={S} n={n} {dtype} mask={su_mask}')
    cpu32.backward(g)
    assert grad.dtype == dtype
    err = float((grad.float() - l32.grad).abs().max())
    assert err <= _grad_tol(dtype) * max(1.0, float(l32.grad.abs().max())), err
    assert torch.all(grad[~row_on] == 0)                              # padded / masked-out rows
    if su_mask:
        no_end = torch.arange(S)[None] < (lengths - 1).clamp(min=0)[:, None]
        other = torch.where(no_end, labels, torch.full_like(labels, n))
        forbid = torch.zeros(b, n + 1, dtype=torch.bool).scatter_(1, other, True)[:, None].expand(b, S, n + 1).clone()
        forbid.scatter_(2, other[:, :, None], False)
        forbid = forbid[:, :, :n] & row_on[:, :, None]
        assert int(forbid.sum()) > 0
        assert torch.all(grad[forbid] == 0)                           # forbidden columns


# ------------------------------------------------------------------------------------------ tail
def _tail_inputs(b, with_preds, zero_head=None):
    g = torch.Generator().manual_seed(b + 17)
    S, n = 64, 513
    width = (327, 128, 2, n, 24320)
    losses = [4 * torch.rand(b, generator=g) for _ in range(5)]
    labels = [torch.randint(0, c, (b,), generator=g) for c in width]
    amaxes = [torch.where(torch.rand(b, generator=g) < 0.5, lab, torch.randint(0, c, (b,), generator=g))
              for lab, c in zip(labels, width)]
    masks = [torch.rand(b, generator=g) > 0.3 for _ in range(5)]
    if zero_head is not None:
        masks[zero_head] = torch.zeros(b, dtype=torch.bool)
    for f in range(1, 5):                     # switched-off rows carry loss 0 and argmax -1, as sl_head_ce leaves them
        losses[f] = losses[f] * masks[f]
        amaxes[f] = torch.where(masks[f], amaxes[f], torch.full_like(amaxes[f], -1))
    su_len = torch.randint(0, S + 1, (b,), generator=g)
    su_on = torch.rand(b, generator=g) > 0.3
    ent = torch.randint(S + 8, n, (b,), generator=g)
    su_lab = torch.randint(0, S + 8, (b, S), generator=g)             # a narrow range: duplicates inside the lists
    for i in range(b):
        if su_len[i] > 0:
            su_lab[i, su_len[i] - 1] = ent[i]
    row_on = (torch.arange(S)[None] < su_len[:, None]) & su_on[:, None]
    su_loss = 3 * torch.rand(b, S, generator=g) * row_on
    preds = ent_in = None
    if with_preds:
        preds = torch.where(torch.rand(b, S, generator=g) < 0.6, su_lab, torch.randint(0, S + 8, (b, S), generator=g))
        preds[0] = torch.randint(0, S + 8, (S,), generator=g)          # no end flag predicted
        ent_in = ent
    w = torch.tensor([30.0, 9.0, 1.0, 4.0, 4.0, 8.0])
    return dict(losses=losses, argmaxes=amaxes, labels=labels, masks=masks, su_loss=su_loss, su_labels=su_lab,
                su_len=su_len, su_on=su_on, preds=preds, ent_num=ent_in, w=w, n=n)


def _run_tail(fn, t, cr, dtype, device):
    mv = lambda x: None if x is None else x.to(device)  # noqa: E731
    losses = [x.to(device, dtype).requires_grad_(True) for x in t['losses']]
    su_loss = t['su_loss'].to(device, dtype).requires_grad_(True)
    total, info = fn(losses, [mv(x) for x in t['argmaxes']], [mv(x) for x in t['labels']],
                     [mv(x) for x in t['masks']], su_loss, mv(t['su_labels']), mv(t['su_len']), mv(t['su_on']),
                     mv(t['preds']), mv(t['ent_num']), t['w'].to(device, dtype),
                     torch.tensor([cr], dtype=dtype, device=device), t['n'])
    grads = torch.autograd.grad(total, losses + [su_loss])
    return info.detach().cpu(), [x.detach().cpu() for x in grads]


LOSS_SLOTS = (0, 1, 2, 3, 4, 5, 6, 7, 14)
METRIC_SLOTS = (8, 9, 10, 11, 12, 13)


@pytest.mark.parametrize('cr', [0.0, 2.0 / 777.0])
@pytest.mark.parametrize('with_preds', [True, False])
@pytest.mark.parametrize('b', [1, 6, 384])
def test_sl_loss_tail_matches_float64(b, with_preds, cr):
    t = _tail_inputs(b, with_preds)
    cr32 = float(np.float32(cr))
    want, want_g = _run_tail(R.sl_loss_tail, t, cr32, torch.float64, 'cpu')
    t32, _ = _run_tail(R.sl_loss_tail, t, cr32, torch.float32, 'cpu')
    got, got_g = _run_tail(ops.sl_loss_tail, t, cr32, torch.float32, DEV)
    again, again_g = _run_tail(ops.sl_loss_tail, t, cr32, torch.float32, DEV)
    assert got.shape == (15,) and bool(torch.isfinite(got).all())
    assert torch.equal(got, again) and all(torch.equal(a, c) for a, c in zip(got_g, again_g))   # the same bits
    for i in LOSS_SLOTS:
        ek, et = abs(float(got[i]) - float(want[i])), abs(float(t32[i]) - float(want[i]))
        print(R.SL_INFO_KEYS[i], 'kernel err', ek, 'torch err', et)
        assert ek <= max(4 * et, _ulp(float(want[i]))), R.SL_INFO_KEYS[i]
    for i in METRIC_SLOTS:
        assert abs(float(got[i]) - float(want[i])) <= 1e-6 * max(abs(float(want[i])), 1e-30) or \
            float(got[i]) == float(want[i]), R.SL_INFO_KEYS[i]
    if with_preds:
        assert float(want[11]) > 0
    else:
        assert float(got[11]) == 0.0
    # a row gradient is one fp32 rounding of w / count (or w cr): 1e-6 relative is 16 ulp
    for a, c in zip(got_g, want_g):
        assert a.dtype == torch.float32
        assert float((a.double() - c).abs().max()) <= 1e-6 * float(c.abs().max())


@pytest.mark.parametrize('cr', [0.0, 0.25])
def test_sl_loss_tail_all_zero_mask(cr):
    t = _tail_inputs(6, True, zero_head=3)
    got, got_g = _run_tail(ops.sl_loss_tail, t, cr, torch.float32, DEV)
    assert bool(torch.isfinite(got).all())
    assert float(got[4]) == 0.0 and float(got[12]) == 0.0            # target_unit: info slots 4 (loss), 12 (accuracy)
    assert torch.all(got_g[3] == 0)
    assert all(bool(torch.isfinite(x).all()) for x in got_g)


# ------------------------------------------------------------------------------------------ SupervisedLoss end to end
@pytest.fixture(scope='module')
def sl_case():
    """Model.sl_train on sl_batch(2, 3, max_entities=30): the logits in fp32 and under bf16 autocast, computed once."""
    from applestar_amd.models.model import Model
    from applestar_amd.rl.synthetic import sl_batch, to_device
    torch.manual_seed(0)
    m = Model({}).to(DEV)
    batch = to_device(sl_batch(2, 3, max_entities=30, seed=4), DEV)
    kw = {k: v for k, v in batch.items() if k != 'new_episodes'}
    out = {'batch': batch}
    with torch.no_grad():
        out['fp32'] = m.sl_train(**kw)[:2]
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out['bf16'] = m.sl_train(**kw)[:2]
    return out


def _run_loss(sl_case, precision, cfg, monkeypatch, fused):
    monkeypatch.setattr(L, 'FUSED_SL_LOSS', fused)
    logits, act = sl_case[precision]
    b = sl_case['batch']
    lg = {k: v.detach().clone().requires_grad_(True) for k, v in logits.items()}
    out = SupervisedLoss(cfg).compute_loss(lg, b['action_info'], b['action_mask'], b['selected_units_num'],
                                           b['entity_num'], act)
    grads = torch.autograd.grad(out['total_loss'], [lg[h] for h in HEADS])
    return out, dict(zip(HEADS, grads))


def _compare_paths(sl_case, precision, cfg, monkeypatch):
    fused, gf = _run_loss(sl_case, precision, cfg, monkeypatch, True)
    plain, gp = _run_loss(sl_case, precision, cfg, monkeypatch, False)
    assert set(fused) == set(plain)
    for k, v in plain.items():
        assert abs(float(fused[k]) - float(v)) <= 1e-4 * max(1.0, abs(float(v))), k
        if k != 'total_loss':
            assert not fused[k].requires_grad, k
    for h in HEADS:
        assert gf[h].dtype == gp[h].dtype == sl_case[precision][0][h].dtype
        err = float((gf[h].float() - gp[h].float()).abs().max())
        assert err <= _grad_tol(gf[h].dtype) * max(1.0, float(gp[h].float().abs().max())), (h, err)
    return fused, plain


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_supervised_loss_fused_matches_torch(sl_case, precision, monkeypatch):
    calls = []
    real = ops.sl_head_ce
    monkeypatch.setattr(ops, 'sl_head_ce', lambda *a, **k: calls.append(1) or real(*a, **k))
    _compare_paths(sl_case, precision, {}, monkeypatch)
    assert len(calls) == 6                                            # the fused path ran: six launches, once


def test_supervised_loss_fused_label_smooth(sl_case, monkeypatch):
    fused, _ = _compare_paths(sl_case, 'fp32', {'label_smooth': True}, monkeypatch)
    base, _ = _run_loss(sl_case, 'fp32', {}, monkeypatch, True)
    assert abs(float(fused['delay_loss']) - float(base['delay_loss'])) > 1e-4


def test_supervised_loss_fused_cross_rank(sl_case, monkeypatch):
    fused, _ = _compare_paths(sl_case, 'fp32', {'cross_rank_loss': True}, monkeypatch)
    base, _ = _run_loss(sl_case, 'fp32', {}, monkeypatch, True)
    assert abs(float(fused['total_loss']) - float(base['total_loss'])) > 1e-3


def test_supervised_loss_without_the_kernels_runs_torch(sl_case, monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the fused path ran')
    monkeypatch.setattr(N, '_IMPLEMENTED', N._IMPLEMENTED - {'sl_loss'})
    monkeypatch.setattr(ops, 'sl_head_ce', boom)
    out, _ = _run_loss(sl_case, 'fp32', {}, monkeypatch, True)
    assert bool(torch.isfinite(out['total_loss']))


# ------------------------------------------------------------------------------------------ one trainer step
def _trainer_step(monkeypatch, fused):
    from applestar_amd.rl.synthetic import sl_batch, to_device
    from applestar_amd.sl.trainer import SLTrainer
    monkeypatch.setattr(L, 'FUSED_SL_LOSS', fused)
    torch.manual_seed(3)
    tr = SLTrainer({'learner': {'ignore_steps': 0, 'data': {'batch_size': 2, 'trajectory_length': 3}}}, device=DEV)
    batch = to_device(sl_batch(2, 3, max_entities=30, seed=1), DEV)
    info = tr.step(batch)
    # the trainer's backward fills flat buckets (unused slots zeroed), so which parameters the loss reaches is
    # asked of autograd directly, on a second forward of the same model
    kw = {k: v for k, v in batch.items() if k not in ('new_episodes', 'hidden_state')}
    logits, act, _ = tr.model.sl_train(**kw, hidden_state=tr.hidden_state)
    out = tr.loss.compute_loss(logits, batch['action_info'], batch['action_mask'], batch['selected_units_num'],
                               batch['entity_num'], act)
    named = [(n, p) for n, p in tr.model.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out['total_loss'], [p for _, p in named], allow_unused=True)
    got_grad = {n for (n, _), g in zip(named, grads) if g is not None}
    return info['total_loss'].detach().clone(), got_grad


def test_sl_trainer_step_with_the_fused_loss(monkeypatch):
    prev = ops.set_deterministic(True)
    try:
        t1, g1 = _trainer_step(monkeypatch, True)
        t2, _ = _trainer_step(monkeypatch, True)
        t0, g0 = _trainer_step(monkeypatch, False)
    finally:
        ops.set_deterministic(prev)
    assert bool(torch.isfinite(t1))
    assert torch.equal(t1, t2)                                        # two fresh trainers, one seed: the same bits
    assert g0 <= g1 and len(g0) > 0
    assert abs(float(t1) - float(t0)) <= 1e-4 * max(1.0, abs(float(t0)))
