"""The deterministic mode on the GPU (``ops.set_deterministic`` / ``APPLESTAR_DETERMINISTIC=1``): every ordered
kernel returns the same bits launch after launch - with the allocator handing out different blocks and with
another stream keeping the device busy - and stays within the accuracy bound of the atomic kernel it replaces.

Inputs are built to collide (many sources per destination) with random signs and magnitudes from 1e-3 to 1e3, so
that any change of the summation order changes the low bits of a sum."""
import pytest
import torch

from applestar_amd import ops
from applestar_amd.ops import native as N
from applestar_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _deterministic_mode():
    N.ensure_loaded()
    prev = N.set_deterministic(True)
    yield
    N.set_deterministic(prev)


def _wide(*shape, seed=0, dtype=torch.float32):
    """Random sign, magnitude 10^U(-3, 3)."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (6.0 * torch.rand(*shape, generator=g) - 3.0)
    sign = torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).to(dtype).to(DEV)


def _churn(i):
    """Shift what the caching allocator hands out next: blocks of odd sizes allocated, some kept, some freed."""
    keep = [torch.empty(1000 * (i + 1) + 17 * k, device=DEV) for k in range(1, 6)]
    del keep[::2]
    if i % 3 == 2:
        torch.cuda.empty_cache()
    return keep


def _reproducible(fn):
    """fn() -> tuple of tensors.  Eight launches with allocator churn in between, then one more while a matmul loop
    runs on a side stream: all bit-identical.  Returns the first result."""
    held, outs = [], []
    for i in range(8):
        held.append(_churn(i))
        outs.append(tuple(t.clone() for t in fn()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            a = (a @ a).clamp_(-1.0, 1.0)
    busy = fn()
    torch.cuda.synchronize()
    for x, y in zip(outs[0], busy):
        assert torch.equal(x, y)
    return outs[0]


# ------------------------------------------------------------------ small-table gradients
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('U,V,D', [(5000, 5, 8), (300, 3, 64)])
def test_table_grad_ordered(U, V, D, dtype):
    """table_grad in its ordered form (fixed row ranges per workgroup + column_reduce), indices outside [0, V)
    included (skipped); accuracy bound of test_kernels_gpu.test_segment_sum_and_gather_rows."""
    C = N.ensure_loaded()
    src = _wide(U, D, seed=U, dtype=dtype)
    idx = torch.randint(-1, V + 1, (U,), generator=torch.Generator().manual_seed(1)).to(DEV)
    out, = _reproducible(lambda: (C.table_grad(src, idx, V, True),))
    ok = ((idx >= 0) & (idx < V)).cpu()
    ref = torch.zeros(V, D, dtype=torch.float64).index_add(0, idx.cpu()[ok], src.cpu().double()[ok])
    assert out.dtype == torch.float32
    assert (out.cpu().double() - ref).abs().max().item() < 1e-3 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('idt', [torch.int64, torch.uint8])
@pytest.mark.parametrize('U,V,D', [(5000, 5, 8), (300, 3, 64), (30, 3, 64)], ids=['multi8', 'multi64', 'direct'])
def test_embed_relu_bwd_ordered(U, V, D, idt, dtype):
    """embed_relu_bwd in its ordered form: the one-workgroup direct path (U * D <= 2048) and the multi-workgroup
    path; indices past the table are clamped; accuracy bound of test_glue_fusions_gpu.test_embed_relu_matches_torch."""
    C = N.ensure_loaded()
    table = torch.randn(V, D, generator=torch.Generator().manual_seed(2)).to(dtype).to(DEV)
    idx = torch.randint(0, V + 3, (U,), generator=torch.Generator().manual_seed(3)).to(idt).to(DEV)
    out = C.embed_relu_fwd(table, idx)
    dout = _wide(U, D, seed=U + 1, dtype=dtype)
    dtab, = _reproducible(lambda: (C.embed_relu_bwd(dout, out, idx, V, True),))
    ic = idx.long().clamp(max=V - 1).cpu()
    mask = (table.cpu().float()[ic] > 0).double()
    ref = torch.zeros(V, D, dtype=torch.float64).index_add(0, ic, dout.cpu().double() * mask)
    assert (dtab.cpu().double() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())


def test_small_table_ops_dispatch_to_ordered_kernels():
    """ops.gather_rows / ops.embed_relu take the ordered backward when the mode is on: the table gradients equal
    the ordered kernels' bits."""
    C = N.ensure_loaded()
    U, V, D = 5000, 5, 8
    idx = torch.randint(0, V, (U,), generator=torch.Generator().manual_seed(4)).to(DEV)
    g = _wide(U, D, seed=9)
    t = torch.randn(V, D, device=DEV, requires_grad=True)
    ops.gather_rows(t, idx).backward(g)
    assert torch.equal(t.grad, C.table_grad(g, idx, V, True))
    t2 = torch.randn(V, D, device=DEV, requires_grad=True)
    out = ops.embed_relu(t2, idx)
    out.backward(g)
    assert torch.equal(t2.grad, C.embed_relu_bwd(g, out.detach(), idx, V, True))


# ------------------------------------------------------------------ selected-units gather
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_gather_steps_backward_bit_equals_ordered_reference(dtype):
    """ops.gather_steps: forward == torch.gather; backward bit-equal to reference.gather_steps_grad_ordered (fp32 sums
    in ascending step).  Labels with triple duplicates and one observation whose labels are all the end index."""
    B, N1, S, C = 3, 10, 12, 32
    labels = torch.tensor([[4, 1, 4, 7, 4, 1, 0, 1, 2, 7, 7, 3],
                           [N1 - 1] * S,
                           [0, 0, 0, 5, 6, 5, 8, 5, 2, 2, 2, 9]], device=DEV)
    key = _wide(B, N1, C, seed=5, dtype=dtype).requires_grad_()
    dout = _wide(B, S, C, seed=6, dtype=dtype)

    def run():
        key.grad = None
        out = ops.gather_steps(key, labels)
        out.backward(dout)
        return out.detach(), key.grad

    out, dkey = _reproducible(run)
    assert torch.equal(out, key.detach().gather(1, labels.unsqueeze(-1).expand(B, S, C)))
    want = R.gather_steps_grad_ordered(dout.cpu(), labels.cpu(), N1)
    assert dkey.dtype == dtype and torch.equal(dkey.cpu(), want)
    assert float(dkey[1, :N1 - 1].abs().max()) == 0.0          # rows no label names
    # float64: at most S - 1 roundings of partial sums bounded by sum |terms|, plus the final bf16 rounding (unit
    # roundoff 2^-8)
    oh = torch.nn.functional.one_hot(labels.cpu(), N1).double()                      # [B,S,N1]
    ref = torch.einsum('bsn,bsc->bnc', oh, dout.cpu().double())
    mag = torch.einsum('bsn,bsc->bnc', oh, dout.cpu().double().abs())
    eps = 2.0 ** -24 * (S - 1) + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    assert bool(((dkey.cpu().double() - ref).abs() <= eps * mag).all())


def test_index_rows_backward_is_ordered():
    """ops.index_rows (the heads' one-hot-times-weight column gathers and the embedding tables too large for
    table_grad's LDS copies; default: index_select with torch's atomic index_add_ backward): forward == index_select,
    table gradient bit-equal to the ordered reference with the whole batch as one observation - more rows than one
    staged chunk of labels, many rows per table entry, through a transposed (non-contiguous) weight view."""
    V, D, U = 327, 256, 2500
    w = _wide(D, V, seed=21).requires_grad_()                        # a Linear weight [out, in]: the table is w.t()
    idx = torch.randint(0, 12, (U,), generator=torch.Generator().manual_seed(22)).to(DEV) * 29
    g = _wide(U, D, seed=23)

    def run():
        w.grad = None
        out = ops.index_rows(w.t(), idx)
        out.backward(g)
        return out.detach(), w.grad

    out, dw = _reproducible(run)
    assert torch.equal(out, w.detach().t().index_select(0, idx))
    want = R.gather_steps_grad_ordered(g.cpu()[None], idx.cpu()[None], V)[0]
    assert torch.equal(dw.cpu(), want.t())


# ------------------------------------------------------------------ value-encoder scatter connection
def _scatter_case(idt):
    B, U, C, H, W = 3, 70, 8, 8, 10
    g = torch.Generator().manual_seed(7)
    x = torch.zeros(B, U, dtype=torch.int64)
    y = torch.zeros(B, U, dtype=torch.int64)
    # observation 0: every unit on one of two pixels, one of them named by coordinates past the map (clamped)
    far = torch.rand(U, generator=g) < 0.5
    x[0] = torch.where(far, 120, 3)
    y[0] = torch.where(far, 100, 2)
    # observation 1: no two units share a pixel
    perm = torch.randperm(H * W, generator=g)[:U]
    x[1], y[1] = perm % W, perm // W
    # observation 2: total_unit_count = 0 (every row masked to zero), coordinates arbitrary
    x[2] = torch.randint(0, W, (U,), generator=g)
    y[2] = torch.randint(0, H, (U,), generator=g)
    count = torch.tensor([U, U, 0])
    return B, U, C, H, W, x.to(idt).to(DEV), y.to(idt).to(DEV), count.to(DEV)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('idt', [torch.int64, torch.uint8])
def test_scatter_connection_bit_equals_ordered_reference(idt, dtype):
    """ops.scatter_connection in deterministic mode: forward bit-equal to reference.scatter_connection_ordered,
    backward equal to the gather of the map gradient at each unit's (clamped) pixel."""
    B, U, C, H, W, x, y, count = _scatter_case(idt)
    mask = ops.sequence_mask(count, U).unsqueeze(-1)
    proj = (_wide(B, U, C, seed=8, dtype=dtype) * mask.to(dtype)).requires_grad_()
    dmap = _wide(B, C, H, W, seed=9, dtype=dtype)

    def run():
        proj.grad = None
        sc = ops.scatter_connection(proj, x, y, H, W)
        sc.backward(dmap)
        return sc.detach(), proj.grad

    sc, dproj = _reproducible(run)
    assert sc.shape == (B, C, H, W) and sc.permute(0, 2, 3, 1).is_contiguous() and sc.dtype == dtype
    want = R.scatter_connection_ordered(proj.detach().cpu(), x.cpu(), y.cpu(), H, W)
    assert torch.equal(sc.cpu(), want)
    assert float(sc[2].abs().max()) == 0.0
    assert int((sc[0].abs().sum(0) > 0).sum()) == 2                     # two pixels, one of them the clamped corner
    assert float(sc[0, :, H - 1, W - 1].abs().max()) > 0.0
    xi, yi = x.long().clamp(0, W - 1), y.long().clamp(0, H - 1)
    bi = torch.arange(B, device=DEV)[:, None].expand(B, U)
    assert torch.equal(dproj, dmap[bi, :, yi, xi])
    # float64, on the atomic form's terms: index_add_ of the same rows (bounded like the gather above)
    ref = R.scatter_connection(proj.detach().cpu().double(), x.cpu(), y.cpu(), H, W)
    mag = R.scatter_connection(proj.detach().cpu().double().abs(), x.cpu(), y.cpu(), H, W)
    eps = 2.0 ** -24 * (U - 1) + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    assert bool(((sc.cpu().double() - ref).abs() <= eps * mag).all())


def test_scatter_connection_feeds_the_fused_value_projection():
    """The ordered scatter map is accepted by the fused consumer (value_spatial_proj_pool) at H x W = 8 x 10, and
    the gradient reaches the unit rows through both native nodes."""
    B, U, C, H, W, x, y, count = _scatter_case(torch.int64)
    proj = torch.randn(B, U, C, device=DEV).relu().requires_grad_()
    own = torch.rand(B, 1, H, W, device=DEV) < 0.2
    enemy = torch.rand(B, 1, H, W, device=DEV) < 0.2
    w = (0.3 * torch.randn(16, 10, 1, 1, device=DEV)).requires_grad_()
    b = (0.1 * torch.randn(16, device=DEV)).requires_grad_()
    sc = ops.scatter_connection(proj, x, y, H, W)
    pooled = ops.value_spatial_proj_pool(sc, own, enemy, w, b)
    assert pooled is not None and pooled.shape == (B, 16, H // 2, W // 2)
    full = torch.relu(torch.nn.functional.conv2d(torch.cat([sc.detach(), own.float(), enemy.float()], 1),
                                                 w.detach(), b.detach()))
    want = torch.nn.functional.max_pool2d(full, 2, 2)
    assert (pooled - want).abs().max().item() < 1e-2 * max(1.0, want.abs().max().item())
    pooled.sum().backward()
    assert proj.grad is not None and bool(torch.isfinite(proj.grad).all()) and float(proj.grad.abs().max()) > 0.0


# ------------------------------------------------------------------ RL loss statistics
@pytest.mark.parametrize('fields', [1, 2])
def test_rl_loss_ordered_statistics(fields):
    """rl_loss.hip with ordered sums: the info vector, the total and every gradient bit-identical over the
    launches; against the torch loss path at the bounds of test_model_gpu.test_fused_rl_loss_matches_torch_loss.
    T = 8, B = 4; winloss alone (the bench's fields) and winloss + build_order (more than one field per lane)."""
    from applestar_amd.rl import loss as L
    from applestar_amd.rl.synthetic import rl_batch, to_device
    dev = torch.device('cuda')
    T, B = 8, 4
    batch = to_device(rl_batch(B, T, max_entities=40, seed=3), dev)
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)  # noqa: E731
    logits = {}
    for i, (h, t) in enumerate(batch['teacher_logit'].items()):
        xh = t + 0.5 * torch.randn(t.shape, device=dev, generator=gen(10 + i))
        logits[h] = torch.where(t > -1e8, xh, torch.full_like(xh, -1e9)).requires_grad_()
    values = {'winloss': (0.3 * torch.randn(T + 1, B, device=dev, generator=gen(1))).requires_grad_()}
    mask = dict(batch['mask'])
    cfg = {}
    if fields == 2:
        values['build_order'] = (0.3 * torch.randn(T + 1, B, device=dev, generator=gen(2))).requires_grad_()
        mask['build_order_mask'] = (torch.rand(T, B, device=dev, generator=gen(7)) < 0.7).float()
        cfg = {'loss_weights': {'pg': {'build_order': 0.5}, 'baseline': {'build_order': 2.0}}}
    inp = {'target_logit': logits, 'value': values, 'action_log_prob': batch['behaviour_logp'],
           'teacher_logit': batch['teacher_logit'], 'mask': mask, 'action': batch['action_info'],
           'reward': batch['reward'], 'step': batch['step']}
    leaves = list(logits.values()) + list(values.values())
    loss = L.ReinforcementLoss(cfg)
    keys = []

    def run():
        info = loss.compute_loss(dict(inp))
        grads = torch.autograd.grad(info['total_loss'], leaves, allow_unused=True)
        keys[:] = sorted(info)
        return tuple(info[k].detach().reshape(()) for k in keys) + \
            tuple(torch.zeros_like(p) if g is None else g for g, p in zip(grads, leaves))

    assert loss._fused_ok(inp)
    got = _reproducible(run)
    L.FUSED_LOSS = False
    try:
        tinfo = L.ReinforcementLoss(cfg).compute_loss(dict(inp))
        tgrads = torch.autograd.grad(tinfo['total_loss'], leaves, allow_unused=True)
    finally:
        L.FUSED_LOSS = True
    assert set(keys) == set(tinfo)
    for k, a in zip(keys, got):
        r = float(tinfo[k].detach()) if torch.is_tensor(tinfo[k]) else float(tinfo[k])
        assert abs(float(a) - r) <= 1e-4 + 1e-4 * abs(r), (k, float(a), r)
    for a, r in zip(got[len(keys):], tgrads):
        if r is None:
            assert float(a.abs().max()) == 0.0
            continue
        assert float((a - r).abs().max()) <= 1e-5 + 1e-4 * float(r.abs().max())


# ------------------------------------------------------------------ policy spatial embedding
def _spatial_case():
    """16 x 20 pixels = two 256-pixel tiles (the second partial).  Observation 0: 280 entities on 3 pixels of tile 0
    (more than the 256-entry list: a second round), 20 more anywhere; observation 1: 40 of N = 300 valid, a few
    sharing a pixel."""
    from applestar_amd.lib.features import SPATIAL_ONE_HOT, EFFECT_KEYS
    g = torch.Generator().manual_seed(12)
    B, H, W, Nn, L = 2, 16, 20, 300, 5
    sp = {'height_map': torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)}
    for k, n in SPATIAL_ONE_HOT:
        sp[k] = torch.randint(0, n + 1, (B, H, W), generator=g, dtype=torch.uint8)
    for k in EFFECT_KEYS:
        sp[k] = torch.randint(0, H * W, (B, L), generator=g, dtype=torch.int16)
    ex = torch.randint(0, W, (B, Nn), generator=g)
    ey = torch.randint(0, H, (B, Nn), generator=g)
    spots = torch.tensor([[3, 1], [19, 5], [0, 12]])                 # (x, y): pixels 23, 119, 240 of tile 0
    pick = torch.randint(0, 3, (280,), generator=g)
    ex[0, :280], ey[0, :280] = spots[pick, 0], spots[pick, 1]
    ex[1, :40] = torch.randint(0, 6, (40,), generator=g)            # 40 entities on 6 x 5 pixels: collisions
    ey[1, :40] = torch.randint(11, 16, (40,), generator=g)          # rows of the second tile too
    en = torch.tensor([Nn, 40])
    rows = _wide(B, Nn, 32, seed=13).cpu() * (torch.arange(Nn)[None] < en[:, None]).unsqueeze(2)
    w = torch.randn(32, 24, generator=g) * 0.3
    b = torch.randn(32, generator=g) * 0.1
    return sp, ex, ey, en, rows, w, b


def _spatial_reference(sp, ex, ey, en, rows, w, b):
    """float64 relu(pre) [B, 32, H, W] of the planes + the entity rows."""
    from applestar_amd.lib.features import SPATIAL_ONE_HOT, EFFECT_KEYS
    B, H, W = sp['height_map'].shape
    planes = [sp['height_map'].double().unsqueeze(1) / 256]
    for k, n in SPATIAL_ONE_HOT:
        planes.append(torch.nn.functional.one_hot(sp[k].long().clamp(0, n - 1), n).permute(0, 3, 1, 2).double())
    for k in EFFECT_KEYS:
        m = torch.zeros(B, H * W, dtype=torch.float64)
        m.scatter_(1, sp[k].long(), 1.0)
        planes.append(m.view(B, 1, H, W))
    pre = torch.einsum('bkhw,nk->bnhw', torch.cat(planes, 1), w.double()) + b.double()[None, :, None, None]
    for i in range(B):
        for j in range(int(en[i])):
            pre[i, :, ey[i, j], ex[i, j]] += rows[i, j].double()
    return torch.relu(pre)


@pytest.mark.parametrize('fp32', [True, False], ids=['fp32', 'bf16'])
def test_spatial_embed_ordered(fp32):
    """spatial_embed and its pooled form with the entity rows added in ascending entity index by a fixed owner
    thread: bit-identical launches; accuracy bounds of test_kernels_gpu.test_spatial_embed_partial_tile (1e-5 fp32,
    2e-2 bf16, relative to the map's maximum)."""
    sp, ex, ey, en, rows, w, b = _spatial_case()
    rows_in = rows if fp32 else rows.to(torch.bfloat16)
    ref = _spatial_reference(sp, ex, ey, en, rows_in.float(), w, b)
    spd = {k: v.to(DEV) for k, v in sp.items()}
    exd, eyd, end, rd, wd, bd = (t.to(DEV) for t in (ex, ey, en, rows_in, w, b))

    def run():
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=not fp32):
            full = N.spatial_embed(spd, rd, exd, eyd, end, wd, bd)
            pooled = N.spatial_embed_pool(spd, rd, exd, eyd, end, wd, bd)
        assert pooled is not None
        return full, pooled

    full, pooled = _reproducible(run)
    assert full.dtype == pooled.dtype == (torch.float32 if fp32 else torch.bfloat16)
    tol = (1e-5 if fp32 else 2e-2) * max(1.0, float(ref.abs().max()))
    assert (full.cpu().double() - ref).abs().max().item() < tol
    assert (pooled.cpu().double() - torch.nn.functional.max_pool2d(ref, 2, 2)).abs().max().item() < tol


# ------------------------------------------------------------------ build-order encoder backward
@pytest.mark.parametrize('wdtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_bo_encoder_backward_ordered(wdtype):
    """The build-order encoder's backward with one workgroup per gradient replica walking its observations in
    order (70 observations on 32 replicas; tokens repeat actions and positions inside an observation): every
    parameter gradient bit-identical over the launches; against the op-by-op module in float64 at the bounds of
    test_kernels_gpu.test_bo_encoder_fused_matches_torch."""
    import torch.nn.functional as F
    from applestar_amd.models.encoders import BeginningBuildOrderEncoder, SPATIAL_X
    torch.manual_seed(31)
    enc = BeginningBuildOrderEncoder(64).to(DEV)
    if wdtype == torch.bfloat16:
        for i, p in enumerate(enc.fused_params()):
            if not (i >= 2 and (i - 2) % 12 in (0, 1, 6, 7)):
                p.data = p.data.to(torch.bfloat16)
    ref = BeginningBuildOrderEncoder(64)
    ref.load_state_dict({k: v.float().cpu() for k, v in enc.state_dict().items()})
    ref = ref.double()
    B, L = 70, 20
    g = torch.Generator().manual_seed(32)
    bo = torch.randint(0, 6, (B, L), generator=g)                       # 6 actions over 20 tokens: repeats
    loc = torch.randint(0, 4, (B, L), generator=g) * 1601 + 7           # 4 positions: repeated coordinate bits
    bo[5, 3:] = 0
    gout = torch.randn(B, 64, generator=g)
    bod, locd, gd = bo.to(DEV), loc.to(DEV), gout.to(DEV)
    assert enc._fusable(bod)
    params = [p for p in enc.parameters()]

    def run():
        for p in params:
            p.grad = None
        out = enc(bod, locd)
        out.float().backward(gd)
        return (out.detach(),) + tuple(p.grad for p in params if p.grad is not None)

    got = _reproducible(run)
    act = F.one_hot(bo.clamp(0, ref.action_dim - 1), ref.action_dim).double()
    pos = torch.eye(L, dtype=torch.float64).expand(B, L, L)
    lx = ref.location_binary.weight[loc % SPATIAL_X]
    ly = ref.location_binary.weight[torch.div(loc, SPATIAL_X, rounding_mode='floor').clamp(max=1023)]
    x = ref.transformer.forward_dense(torch.cat([act, pos, lx, ly], dim=2))
    out_ref = ref.embedd_fc(x.mean(dim=1))
    out_ref.backward(gout.double())
    tol = 2e-3 if wdtype == torch.float32 else 2e-2
    assert (got[0].cpu().double() - out_ref).abs().max().item() < tol * max(1.0, out_ref.abs().max().item())
    grads = iter(got[1:])
    for pe, pr in zip(params, ref.parameters()):
        if pe.grad is None:
            continue
        a = next(grads)
        assert a.dtype == pe.dtype
        s = pr.grad.abs().max().item()
        assert (a.cpu().double() - pr.grad).abs().max().item() < tol * max(1e-3, s), (tuple(pe.shape), s)


# ------------------------------------------------------------------ the whole learner step
def _poison(val):
    """Fill, then free, blocks of every size class of the caching allocator (tools/diag/poison_probe.py)."""
    torch.cuda.synchronize()
    held = []
    for k in range(8, 28):
        for _ in range(6 if k < 21 else 2):
            held.append(torch.full((1 << (k - 2),), val, device=DEV))
    del held
    torch.cuda.synchronize()


def _trainer(prec, graph=False):
    from applestar_amd.rl.trainer import RLTrainer
    torch.manual_seed(0)
    return RLTrainer({'learner': {'use_value_feature': True, 'amp_dtype': 'bfloat16' if prec == 'bf16' else None,
                                  'graph_step': graph},
                      'model': {'enable_baselines': ['winloss']}}, device='cuda')


def _weights(tr):
    if tr.master is not None:
        return (tr.master.master.detach().clone(),)
    return tuple(p.detach().clone() for p in tr.params)


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_whole_step_is_bit_reproducible(prec):
    """The probe's shape (rl_batch(2, 4, max_entities=48), value feature on, winloss baseline) with the mode on:
    forward + loss + backward three times from the same weights with the allocator's free blocks poisoned in
    between - every head's logits, every value and every parameter gradient bit-identical; then two full steps
    (clip + Adam included) from the same state on two trainers - the updated weights bit-identical."""
    from applestar_amd.rl.synthetic import rl_batch, to_device
    from applestar_amd.runtime.train_engine import amp_context
    tr = _trainer(prec)
    assert N.deterministic()
    batches = [to_device(rl_batch(2, 4, max_entities=48, seed=s), 'cuda') for s in (3, 0)]

    def fwd_bwd():
        tr.model.train()
        with amp_context(tr.device, tr.amp_dtype):
            out = tr.model.rl_learner_forward(**dict(batches[0]))
        info = tr.loss.compute_loss(out)
        tr.backward(info['total_loss'])
        tr._reduce()
        res = {'logit.' + k: v.detach().clone() for k, v in out['target_logit'].items()}
        res.update({'value.' + k: v.detach().clone() for k, v in out['value'].items()})
        res['total_loss'] = info['total_loss'].detach().clone()
        res.update({f'grad.{i}': p.grad.detach().clone() for i, p in enumerate(tr.opt_params) if p.grad is not None})
        torch.cuda.synchronize()
        return res

    fwd_bwd()                                             # warm-up: derived weight forms, side streams
    runs = []
    for val in (0.0, float('nan'), -7.0):
        _poison(val)
        runs.append(fwd_bwd())
    names = {id(p): n for n, p in tr.model.named_parameters()}
    for r in runs[1:]:
        bad = [k if not k.startswith('grad.') else 'grad.' + names.get(id(tr.opt_params[int(k[5:])]), k[5:])
               for k in runs[0] if not torch.equal(runs[0][k], r[k])]
        assert not bad, bad[:12]
    assert sum(float(g.abs().sum()) for k, g in runs[0].items() if k.startswith('grad.')) > 0.0
    other = _trainer(prec)
    for t in (tr, other):
        for b in batches:
            t.step(dict(b))
    torch.cuda.synchronize()
    for a, b in zip(_weights(tr), _weights(other)):
        assert torch.equal(a, b)


def test_whole_step_is_bit_reproducible_in_a_graph():
    """The same with learner.graph_step: first sight of the batch eager, then capture + replay, then replay - every
    ordered kernel is captured (no site raises), and two trainers end with bit-identical weights."""
    from applestar_amd.rl.synthetic import rl_batch, to_device
    from applestar_amd.runtime.prefetch import entity_total_hint
    host = rl_batch(2, 4, max_entities=48, seed=3)
    batch = to_device(host, 'cuda')
    batch['entity_total'] = entity_total_hint(host)
    ends = []
    for _ in range(2):
        tr = _trainer('fp32', graph=True)
        assert tr.graph is not None
        for _ in range(3):
            tr.step(dict(batch))
        torch.cuda.synchronize()
        assert tr.graph.captures == 1 and tr.graph.replays == 2
        ends.append(_weights(tr))
    for a, b in zip(*ends):
        assert torch.equal(a, b)
