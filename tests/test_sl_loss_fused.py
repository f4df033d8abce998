"""The torch definitions behind the fused supervised loss (ops/reference.py sl_head_ce / sl_loss_tail), the
``cross_rank_loss`` option of ``SupervisedLoss`` and a recorded reference run that pins ``label_smooth`` - all on the
CPU."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from refutil import golden
from applestar_amd.ops import reference as ref
from applestar_amd.sl.loss import SupervisedLoss

HEADS = SupervisedLoss.HEADS
FLAT = ref.SL_FLAT_HEADS


# ------------------------------------------------------------------------------------------ per-row cross entropy
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('C', [2, 31])
def test_reference_sl_head_ce_matches_float64(C, eps):
    g = torch.Generator().manual_seed(C)
    R = 6
    x = 3 * torch.randn(R, C, generator=g)
    x[1] = -1e9                                         # a fully masked row
    x[2, 0] = x[2, C - 1] = x[2].max() + 1.0            # two equal maxima: the lower index wins
    lab = torch.randint(0, C, (R,), generator=g)
    loss, amax = ref.sl_head_ce(x, lab, eps)
    lp = torch.log_softmax(x.double(), -1)
    want = -lp.gather(-1, lab[:, None])[:, 0]
    if eps > 0:
        want = (1 - eps) * want + eps * (-lp.mean(-1))
    assert loss.dtype == torch.float32 and amax.dtype == torch.int64
    assert torch.allclose(loss.double(), want, rtol=2e-6, atol=1e-6)
    assert abs(float(loss[1]) - float(torch.log(torch.tensor(float(C))))) < 1e-6 and int(amax[1]) == 0
    assert int(amax[2]) == 0
    for r in (0, 3, 4, 5):
        assert int(amax[r]) == int(x[r].argmax())
    # switched-off rows: not read, loss 0, argmax -1
    on = torch.tensor([1, 1, 0, 1, 0, 1], dtype=torch.bool)
    xp = x.clone()
    xp[~on] = float('nan')
    loss2, amax2 = ref.sl_head_ce(xp, lab, eps, row_on=on)
    assert torch.equal(loss2[on], loss[on]) and torch.equal(amax2[on], amax[on])
    assert torch.all(loss2[~on] == 0) and torch.all(amax2[~on] == -1)


def _su_case():
    """b = 5, S = 7, n = 13: lengths {0, 1, 3, 7, 2}, the end flag (entity_num) at len - 1, one label duplicated
    inside a list, one observation masked out."""
    g = torch.Generator().manual_seed(3)
    b, S, n = 5, 7, 13
    lengths = torch.tensor([0, 1, 3, 7, 2])
    entity_num = torch.tensor([12, 9, 11, 12, 10])
    labels = torch.randint(0, 9, (b, S), generator=g)
    labels[3, :6] = torch.tensor([4, 1, 7, 1, 0, 5])            # unit 1 labelled twice
    for i in range(b):
        if lengths[i] > 0:
            labels[i, lengths[i] - 1] = entity_num[i]
    mask = torch.tensor([True, True, False, True, True])
    logits = 2 * torch.randn(b, S, n, generator=g)
    return logits, labels, mask, lengths, entity_num


@pytest.mark.parametrize('su_mask', [True, False])
def test_reference_selected_units_form_matches_present_code(su_mask):
    logits, labels, mask, lengths, entity_num = _su_case()
    b, S, n = logits.shape
    lg = logits.clone().requires_grad_(True)
    want = SupervisedLoss({'su_mask': su_mask})._selected_units(lg, labels, mask, lengths, entity_num, None)
    lg2 = logits.clone().requires_grad_(True)
    loss, _ = ref.sl_head_ce(lg2, labels, 0.0, su=(lengths, mask), su_mask=su_mask)
    assert loss.shape == (b, S)
    on = (torch.arange(S)[None] < lengths[:, None]) & mask[:, None]
    assert torch.all(loss[~on] == 0)
    assert torch.allclose(loss.sum() / b, want['selected_units_loss'], rtol=1e-6, atol=1e-7)
    ef = loss[torch.arange(b), (lengths - 1).clamp(min=0)].mean()
    assert torch.allclose(ef, want['selected_units_end_flag_loss'], rtol=1e-6, atol=1e-7)
    g1, = torch.autograd.grad(want['selected_units_loss'], lg)
    g2, = torch.autograd.grad(loss.sum() / b, lg2)
    assert torch.allclose(g1, g2, rtol=1e-5, atol=1e-7)
    assert torch.all(g2[~on] == 0)


# ------------------------------------------------------------------------------------------ whole-loss inputs
def _loss_inputs(b, seed=0, dtype=torch.float32):
    """Logits / actions / masks of all six heads for b observations; every head has at least one mask entry zero
    and one set (the action-type mask too, although real batches keep it all ones)."""
    g = torch.Generator().manual_seed(seed)
    S, n = 5, 12
    width = {'action_type': 7, 'delay': 6, 'queued': 2, 'target_unit': n, 'target_location': 480}
    logits, actions, masks = {}, {}, {}
    for h, c in width.items():
        logits[h] = (2 * torch.randn(b, c, generator=g)).to(dtype)
        actions[h] = torch.randint(0, c, (b,), generator=g)
        m = torch.rand(b, generator=g) > 0.4
        m[0], m[1] = True, False
        masks[h] = m
    logits['selected_units'] = (2 * torch.randn(b, S, n, generator=g)).to(dtype)
    entity_num = torch.randint(8, n, (b,), generator=g)
    su_num = torch.randint(0, S + 1, (b,), generator=g)
    lab = torch.zeros(b, S, dtype=torch.long)
    for i in range(b):
        k = int(su_num[i])
        if k > 0:
            lab[i, :k - 1] = torch.randperm(8, generator=g)[:k - 1]
            lab[i, k - 1] = entity_num[i]
    actions['selected_units'] = lab
    m = torch.rand(b, generator=g) > 0.4
    m[0], m[1] = True, False
    masks['selected_units'] = m
    return logits, actions, masks, su_num, entity_num


def test_cross_rank_loss_world_1_normalises_by_the_batch():
    b = 6
    logits, actions, masks, su_num, entity_num = _loss_inputs(b, seed=1)
    plain = SupervisedLoss({}).compute_loss(logits, actions, masks, su_num, entity_num)
    cross = SupervisedLoss({'cross_rank_loss': True}).compute_loss(logits, actions, masks, su_num, entity_num)
    for h in FLAT:
        lp = torch.log_softmax(logits[h].double(), -1)
        nll = -lp.gather(-1, actions[h][:, None])[:, 0]
        want = float((nll * masks[h]).sum() / b)
        assert abs(float(cross[h + '_loss']) - want) <= 2e-6 * max(1.0, abs(want)), h
        assert abs(float(cross[h + '_loss']) - float(plain[h + '_loss'])) > 1e-3, h     # not the masked mean
    assert abs(float(cross['selected_units_loss']) - float(plain['selected_units_loss'])) <= 1e-6
    assert abs(float(cross['total_loss']) - float(plain['total_loss'])) > 1e-2
    for k in ('selected_units_loss_norm', 'selected_units_end_flag_loss', 'action_type_acc', 'delay_distance_L1',
              'queued_acc', 'selected_units_iou', 'target_unit_acc', 'target_location_distance_L2'):
        assert float(cross[k]) == float(plain[k]), k


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rows(tree, lo, hi):
    return {k: v[lo:hi] for k, v in tree.items()}


def _cross_rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    from applestar_amd.parallel import dist as pdist
    pdist.init(backend='gloo')
    logits, actions, masks, su_num, entity_num = _loss_inputs(8, seed=2, dtype=torch.float64)
    lo, hi = (0, 3) if rank == 0 else (3, 8)
    lg = {k: v[lo:hi].clone().requires_grad_(True) for k, v in logits.items()}
    out = SupervisedLoss({'cross_rank_loss': True}).compute_loss(lg, _rows(actions, lo, hi), _rows(masks, lo, hi),
                                                                 su_num[lo:hi], entity_num[lo:hi])
    grads = torch.autograd.grad(out['total_loss'], [lg[h] for h in HEADS])
    q.put({'rank': rank, 'total': out['total_loss'].detach().double().item(),
           'grads': {h: g.double().numpy() for h, g in zip(HEADS, grads)}})
    pdist.finalize()


@pytest.mark.timeout(300)
def test_cross_rank_loss_world_2_averages_to_the_global_batch():
    """Ranks holding 3 and 5 rows of one 8-row batch: the mean over ranks of the loss and of its gradient (rows put
    back in place) is the single-process ``cross_rank_loss`` result on the 8 rows."""
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_cross_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r['rank'])
    for p in procs:
        p.join(timeout=60)
    logits, actions, masks, su_num, entity_num = _loss_inputs(8, seed=2, dtype=torch.float64)
    lg = {k: v.clone().requires_grad_(True) for k, v in logits.items()}
    out = SupervisedLoss({'cross_rank_loss': True}).compute_loss(lg, actions, masks, su_num, entity_num)
    assert out['total_loss'].dtype == torch.float64
    grads = torch.autograd.grad(out['total_loss'], [lg[h] for h in HEADS])
    mean_total = (res[0]['total'] + res[1]['total']) / world
    want_total = float(out['total_loss'].detach())
    assert abs(mean_total - want_total) <= 1e-12 * max(1.0, abs(want_total))
    for h, g in zip(HEADS, grads):
        put_back = torch.cat([torch.from_numpy(res[0]['grads'][h]), torch.from_numpy(res[1]['grads'][h])], 0) / world
        assert float((put_back - g).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max())), h


# ------------------------------------------------------------------------------------------ recorded reference run
@pytest.mark.parametrize('case', ['plain', 'su_mask', 'smooth', 'smooth_su_mask'])
def test_supervised_loss_matches_recorded_reference(case):
    _, ins, outs = golden('sl_loss_reference')
    cfg = {'su_mask': 'su_mask' in case, 'label_smooth': 'smooth' in case}
    mine = SupervisedLoss(cfg).compute_loss(
        {h: ins['logits_' + h] for h in HEADS}, {h: ins['action_' + h] for h in HEADS},
        {h: ins['mask_' + h] for h in HEADS}, ins['selected_units_num'], ins['entity_num'],
        {'selected_units': ins['preds']})
    keys = [k.split('__', 1)[1] for k in outs if k.startswith(case + '__')]
    assert len(keys) == 15
    for k in keys:
        v = float(outs[f'{case}__{k}'])
        assert abs(float(mine[k]) - v) <= 1e-4 * max(1.0, abs(v)), k
    assert float(outs[f'{case}__selected_units_iou']) > 0
    if 'smooth' in case:
        assert abs(float(outs[f'{case}__delay_loss']) - float(outs['plain__delay_loss'])) > 1e-3


# ------------------------------------------------------------------------------------------ tail definition
@pytest.mark.parametrize('cross', [False, True])
def test_reference_tail_matches_supervised_loss(cross):
    """reference.sl_head_ce + reference.sl_loss_tail reproduce every key of the torch ``compute_loss``."""
    _, ins, _ = golden('sl_loss_reference')
    logits = {h: ins['logits_' + h] for h in HEADS}
    actions = {h: ins['action_' + h] for h in HEADS}
    masks = {h: ins['mask_' + h] for h in HEADS}
    su_len, ent = ins['selected_units_num'], ins['entity_num']
    b, S, n = logits['selected_units'].shape
    want = SupervisedLoss({'su_mask': True, 'label_smooth': True, 'cross_rank_loss': cross}).compute_loss(
        logits, actions, masks, su_len, ent, {'selected_units': ins['preds']})
    ce = [ref.sl_head_ce(logits[h], actions[h], 0.1, row_on=None if h == 'action_type' else masks[h]) for h in FLAT]
    su_loss, _ = ref.sl_head_ce(logits['selected_units'], actions['selected_units'], 0.0,
                                su=(su_len, masks['selected_units']), su_mask=True)
    w = torch.tensor([30.0, 9.0, 1.0, 4.0, 4.0, 8.0])
    total, info = ref.sl_loss_tail([c[0] for c in ce], [c[1] for c in ce], [actions[h] for h in FLAT],
                                   [masks[h] for h in FLAT], su_loss, actions['selected_units'], su_len,
                                   masks['selected_units'], ins['preds'], ent, w,
                                   torch.tensor([1.0 / b if cross else 0.0]), n)
    for i, k in enumerate(ref.SL_INFO_KEYS):
        assert abs(float(info[i]) - float(want[k])) <= 1e-5 * max(1.0, abs(float(want[k]))), k
    assert float(total) == float(info[14])
