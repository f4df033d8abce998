"""DAPO on the MI355X: the 4-output ``head_stats`` (KL from the successive model in the same launch), the DAPO
term of the fused loss tail (rl_loss.hip) against the torch loss and a float64 transcription, its ordered form
under the deterministic mode, and the trainer step (eager and graphed) with ``use_dapo``."""
import pytest
import torch

from applestar_amd import ops
from applestar_amd.ops import reference as R
from applestar_amd.ops import native as N
from applestar_amd.rl import rl_utils
from applestar_amd.rl.loss import HEADS
from applestar_amd.rl.synthetic import rl_batch, to_device
from applestar_amd.rl.trainer import RLTrainer

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DAPO_W = {'action_type': 1.0, 'delay': 0.5, 'queued': 2.0, 'selected_units': 0.25, 'target_unit': 1.5,
          'target_location': 0.75}


@pytest.fixture(scope='module', autouse=True)
def _load():
    N.ensure_loaded()


def _err(a, b):
    return (a.float() - b.float()).abs().max().item()


# ---------------------------------------------------------------------------- head_stats, 4 outputs
@pytest.mark.parametrize('C', [2, 327, 4097, 24320])
@pytest.mark.parametrize('ldt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('udt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('with_teacher', [True, False])
def test_head_stats_successive_matches_reference(C, ldt, udt, with_teacher):
    """(logp_a, H, KL_teacher, KL_successive) of one launch and the one-pass backward vs the torch reference in
    fp32: both row mappings (one wave / one workgroup per row), R no multiple of 4, the short tail, the masked
    tail and a fully masked row set in all three tensors; and the 3-output call is untouched by a 4-output one."""
    torch.manual_seed(21)
    Rr = 37
    logits = (3 * torch.randn(Rr, C, device=DEV)).to(ldt)
    teacher = 3 * torch.randn(Rr, C, device=DEV) if with_teacher else None
    succ = (3 * torch.randn(Rr, C, device=DEV)).to(udt)
    if C > 4:
        for x in (logits, teacher, succ):
            if x is not None:
                x[:, C // 2:] = -1e9                # masked tail
                x[3] = -1e9                         # fully masked row
    act = torch.randint(0, max(1, C // 2), (Rr,), device=DEV)
    before = N.head_stats(logits, teacher, act)
    l1 = logits.detach().clone().requires_grad_()
    got = N.head_stats(l1, teacher, act, succ)
    l2 = logits.detach().float().clone().requires_grad_()
    ref = R.head_stats(l2, teacher, act, succ)
    assert len(got) == 4 and len(ref) == 4 and len(before) == 3
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32 and a.shape == b.shape
        assert _err(a, b) < 1e-3 * max(1.0, b.abs().max().item()), _err(a, b)
    if C > 4:
        assert float(got[3][3].detach()) == 0.0     # fully masked: exactly 0, no cancellation at 1e9
    gs = [torch.randn(Rr, device=DEV) for _ in range(4)]
    sum((x * g).sum() for x, g in zip(got, gs)).backward()
    sum((x * g).sum() for x, g in zip(ref, gs)).backward()
    assert l1.grad.dtype == ldt
    tol = 2e-2 if ldt == torch.bfloat16 else 1e-4
    assert _err(l1.grad, l2.grad) < tol * max(1.0, l2.grad.abs().max().item()), _err(l1.grad, l2.grad)
    after = N.head_stats(logits, teacher, act)
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------- fused vs torch loss
def _loss_inputs(T, B, seed=3):
    batch = to_device(rl_batch(B, T, max_entities=40, seed=seed, successive=True), DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    logits = {}
    for i, (h, t) in enumerate(batch['teacher_logit'].items()):
        x = t + 0.5 * torch.randn(t.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(100 + i))
        logits[h] = torch.where(t > -1e8, x, torch.full_like(x, -1e9)).requires_grad_()
    values = {k: (0.3 * torch.randn(T + 1, B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1 + i))
                  ).requires_grad_() for i, k in enumerate(('winloss', 'build_order'))}
    mask = dict(batch['mask'])
    mask['build_order_mask'] = (torch.rand(T, B, device=DEV, generator=g) < 0.7).float()
    return {'target_logit': logits, 'value': values, 'action_log_prob': batch['behaviour_logp'],
            'teacher_logit': batch['teacher_logit'], 'successive_logit': batch['successive_logit'], 'mask': mask,
            'action': batch['action_info'], 'reward': batch['reward'], 'step': batch['step']}


@pytest.mark.parametrize('only_value', [False, True])
@pytest.mark.parametrize('det', [False, True])
def test_fused_rl_loss_with_dapo_matches_torch_loss(only_value, det):
    """The fused path (4-output head_stats + the DAPO form of rl_loss.hip, plain and ordered) vs the torch loss
    with DAPO on: same info keys, every entry, and the gradients of all head logits and baseline values."""
    from applestar_amd.rl import loss as L
    T, B = 16, 3
    inp = _loss_inputs(T, B)
    steps = float(inp['step'].flatten().sort().values[T * B // 2])
    flag = inp['step'] < steps
    assert bool(flag.any()) and not bool(flag.all())                 # the gate is mixed
    cfg = {'loss_weights': {'pg': {'build_order': 0.5}, 'baseline': {'build_order': 2.0}, 'dapo': 0.1},
           'use_dapo': True, 'dapo_head_weights': DAPO_W, 'dapo': {'dapo_steps': steps}}
    results = []
    prev = N.set_deterministic(det)
    try:
        for fused in (True, False):
            L.FUSED_LOSS = fused
            loss = L.ReinforcementLoss(cfg)
            loss.only_update_value = only_value
            assert loss._fused_ok(inp) == fused
            info = loss.compute_loss(dict(inp))
            leaves = list(inp['target_logit'].values()) + list(inp['value'].values())
            results.append((info, torch.autograd.grad(info['total_loss'], leaves, allow_unused=True)))
    finally:
        L.FUSED_LOSS = True
        N.set_deterministic(prev)
    (fi, fg), (ti, tg) = results
    assert set(fi) == set(ti) and 'dapo/total' in fi and all('dapo/' + h in fi for h in HEADS)
    assert float(ti['dapo/total']) > 0
    for k in ti:
        a, r = float(fi[k]), float(ti[k])
        assert abs(a - r) <= 1e-4 + 1e-4 * abs(r), (k, a, r)
    for a, r in zip(fg, tg):
        if r is None:
            assert a is None or float(a.abs().max()) == 0.0
            continue
        a = torch.zeros_like(r) if a is None else a
        assert float((a - r).abs().max()) <= 1e-5 + 1e-4 * float(r.abs().max())


# ---------------------------------------------------------------------------- the tail alone
def _tail_operands(T, B, F, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)   # noqa: E731
    op = {'alp': -3 * ru(6, T, B), 'blp': -3 * ru(6, T, B), 'ent': ru(6, T, B), 'kl': 2 * ru(6, T, B),
          'sk': 2 * ru(6, T, B), 'v': 0.5 * rn(F, T + 1, B), 'r': 0.3 * rn(F, T, B),
          'wm': (ru(F, T, B) < 0.7).double(), 'atflag': (ru(T, B) < 0.5).double(),
          'dflag': (ru(T, B) < 0.5).double()}
    hm = (ru(6, T, B) < 0.6).double()
    hm[:2] = 1.0
    op['hm'] = hm
    sc = {'wpg': ru(F), 'wbase': 2 * ru(F), 'gp': 1 - 0.01 * ru(F), 'gb': 1 - 0.01 * ru(F),
          'pg_w': ru(6), 'upgo_w': ru(6), 'ent_w': ru(6), 'kl_w': ru(6), 'w': ru(4), 'dapo_w': ru(6),
          'w_dapo': ru(1)}
    return op, sc


def _tail_float64(op, sc, upgo_f, only_value):
    """rl/loss.py after the head statistics, in float64 on the host, on the stacked operands of ops.rl_loss_tail:
    (total, per-head dapo means, dapo total, gradients w.r.t. alp, ent, kl, v, sk)."""
    alp, ent, kl, v, sk = (op[k].clone().requires_grad_() for k in ('alp', 'ent', 'kl', 'v', 'sk'))
    hm, r, wm = op['hm'], op['r'], op['wm']
    F = v.shape[0]
    with torch.no_grad():
        rho = torch.exp(alp - op['blp']).clamp(max=1.0)
    total_pg = 0.0
    critic = 0.0
    for f in range(F):
        with torch.no_grad():
            adv = rl_utils.vtrace_advantages(rho, rho, r[f], v[f].detach(), gamma=float(sc['gp'][f]), lambda_=1.0)
        per_head = (-adv * alp * hm * wm[f]).mean(dim=(1, 2))
        total_pg = total_pg + sc['wpg'][f] * (per_head * sc['pg_w']).sum()
        critic = critic + sc['wbase'][f] * rl_utils.td_lambda_loss(v[f], r[f], gamma=float(sc['gb'][f]), lambda_=0.8,
                                                                    weight=wm[f])
    vu = v[upgo_f].detach()
    with torch.no_grad():
        uadv = rho * (rl_utils.upgo_returns(r[upgo_f], vu) - vu[:-1])
    ut = ((-uadv * alp * hm).mean(dim=(1, 2)) * sc['upgo_w']).sum()
    et = -((ent * hm).mean(dim=(1, 2)) * sc['ent_w']).sum()
    kt = ((kl * hm).mean(dim=(1, 2)) * sc['kl_w']).sum()
    at = (kl[0] * op['atflag']).mean()
    d = (sk * hm * op['dflag']).mean(dim=(1, 2))
    dt = (d * sc['dapo_w']).sum()
    w_upgo, w_ent, w_kl, w_at = sc['w']
    total = critic if only_value else \
        total_pg + ut * w_upgo + critic + et * w_ent + kt * w_kl + at * w_at + dt * sc['w_dapo'][0]
    grads = torch.autograd.grad(total, [alp, ent, kl, v, sk], allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, (alp, ent, kl, v, sk))]
    return total.detach(), d.detach(), dt.detach(), grads


def _tail_gpu(op, sc, upgo_f, only_value):
    F = op['v'].shape[0]
    vals = torch.stack([sc['wpg'], sc['wbase'], sc['gp'], sc['gb']], 1).reshape(-1)
    vec = torch.cat([vals, sc['pg_w'], sc['upgo_w'], sc['ent_w'], sc['kl_w'], sc['w'], sc['dapo_w'], sc['w_dapo']])
    assert vec.numel() == 4 * F + 35
    d = {k: x.float().to(DEV) for k, x in op.items()}
    leaves = [d[k].requires_grad_() for k in ('alp', 'ent', 'kl', 'v', 'sk')]
    total, info = ops.rl_loss_tail(d['alp'], d['ent'], d['kl'], d['v'], d['blp'], d['hm'], d['r'], d['wm'],
                                   d['atflag'], vec.float().to(DEV), upgo_f, only_value, d['sk'], d['dflag'])
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    return total.detach(), info.detach(), [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]


def _check_tail(got, ref, F):
    total, info, grads = got
    rtotal, rd, rdt, rgrads = ref
    assert info.numel() == 10 * F + 31 and torch.equal(info[-1], total)
    close = lambda a, r: abs(a - r) <= 1e-4 + 1e-4 * abs(r)  # noqa: E731
    assert close(float(total), float(rtotal)), (float(total), float(rtotal))
    for h in range(6):
        assert close(float(info[-8 + h]), float(rd[h])), (h, float(info[-8 + h]), float(rd[h]))
    assert close(float(info[-2]), float(rdt))
    for name, a, r in zip(('alp', 'ent', 'kl', 'v', 'sk'), grads, rgrads):
        r = r.float().to(DEV)
        assert a.shape == r.shape
        assert float((a - r).abs().max()) <= 1e-5 + 1e-4 * float(r.abs().max()), name


@pytest.mark.parametrize('only_value', [False, True])
def test_rl_loss_tail_dapo_matches_float64(only_value):
    """ops.rl_loss_tail with the DAPO operands at T, B = 4, 64 (6 * B and F * B above 256: phases A and B take
    more than one pass) vs a float64 transcription: total, the seven DAPO entries, all five gradients."""
    T, B, F = 4, 64, 5
    op, sc = _tail_operands(T, B, F, seed=5)
    got = _tail_gpu(op, sc, 1, only_value)
    _check_tail(got, _tail_float64(op, sc, 1, only_value), F)
    if only_value:
        assert float(got[2][4].abs().max()) == 0.0
    else:
        assert float(got[2][4].abs().max()) > 0.0


@pytest.mark.parametrize('T,B,F', [(16, 3, 2), (4, 64, 5)])
def test_rl_loss_tail_dapo_deterministic(T, B, F):
    """Deterministic mode: five launches of the ordered DAPO tail give bit-identical info vectors and gradients,
    within the same bounds of the float64 transcription."""
    op, sc = _tail_operands(T, B, F, seed=9)
    prev = N.set_deterministic(True)
    try:
        runs = [_tail_gpu(op, sc, 0, False) for _ in range(5)]
    finally:
        N.set_deterministic(prev)
    for total, info, grads in runs[1:]:
        assert torch.equal(info, runs[0][1]) and torch.equal(total, runs[0][0])
        for a, b in zip(grads, runs[0][2]):
            assert torch.equal(a, b)
    _check_tail(runs[0], _tail_float64(op, sc, 0, False), F)


# ---------------------------------------------------------------------------- trainer
def _trainer(amp, use_dapo, **lc):
    torch.manual_seed(0)
    return RLTrainer({'learner': dict({'use_value_feature': True, 'amp_dtype': amp, 'use_dapo': use_dapo,
                                       'loss_weights': {'dapo': 0.1}, 'dapo': {'dapo_steps': 4000}}, **lc),
                      'model': {'enable_baselines': ['winloss']}}, device=DEV)


def _flat(tr):
    if tr.master is not None:
        return tr.master.master.detach().clone()
    return torch.cat([p.detach().reshape(-1) for p in tr.params])


@pytest.mark.parametrize('amp', [None, 'bfloat16'])
def test_trainer_steps_with_dapo(amp):
    """Two RLTrainer steps on a batch with successive logits: finite loss, a positive dapo/total in the info, and
    other weights than the same steps with use_dapo off."""
    host = rl_batch(2, 4, max_entities=48, successive=True)
    assert bool((host['step'] < 4000).any())
    on, off = _trainer(amp, True), _trainer(amp, False)
    assert torch.equal(_flat(on), _flat(off))
    for _ in range(2):
        info = on.step(to_device(host, DEV))
        info_off = off.step(to_device(host, DEV))
        assert torch.isfinite(torch.as_tensor(info['total_loss'])).item()
        assert float(info['dapo/total']) > 0
        assert 'dapo/total' not in info_off
    torch.cuda.synchronize()
    assert not torch.equal(_flat(on), _flat(off))


@pytest.mark.parametrize('amp', ['bfloat16', None])
def test_graphed_train_step_with_dapo_matches_eager(amp):
    """The whole-step HIP graph carries the successive logits through its batch refresh: three steps on one batch
    (first sight eager, capture + replay, replay) train like the eager step, at the bounds of
    test_graphed_train_step_matches_eager."""
    from applestar_amd.runtime.prefetch import entity_total_hint
    eager, graphed = _trainer(amp, True), _trainer(amp, True, graph_step=True)
    assert eager.graph is None and graphed.graph is not None
    m0 = _flat(graphed)
    assert torch.equal(m0, _flat(eager))
    host = rl_batch(2, 4, max_entities=48, successive=True)
    b = to_device(host, DEV)
    b['entity_total'] = entity_total_hint(host)
    for i in range(3):
        ie = eager.step(dict(b))
        ig = graphed.step(dict(b))
        for k in ('total_loss', 'gradient', 'dapo/total'):
            a, r = float(ig[k]), float(ie[k])
            assert abs(a - r) <= 2e-2 * max(1.0, abs(r)), (i, k, a, r)
    torch.cuda.synchronize()
    assert graphed.graph.captures == 1 and graphed.graph.replays == 2 and graphed.graph.eager_steps == 1
    de, dg = _flat(eager) - m0, _flat(graphed) - m0
    assert de.abs().max().item() > 0 and dg.abs().max().item() > 0
    cos = float((de * dg).sum() / (de.norm() * dg.norm()))
    assert cos > (0.9 if amp else 0.99), cos
