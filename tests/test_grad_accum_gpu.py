"""Gradient accumulation on the GPU: the native ``multi_accumulate`` / ``multi_strided_accumulate`` launches
(csrc/kernels/multi_copy.hip: ``dst = (dst + src) * scale``, an add and a multiply, fp32 accumulator, fp32 or bf16
source) against the CPU replay, bit for bit; and windows of k micro-batches through the RL trainer
(``backward(more=True)`` ... ``backward``) against the fp32 replay of the single-backward gradients - bit-equal in
the deterministic mode, within the run-to-run noise floor otherwise."""
import copy

import pytest
import torch

from applestar_amd.ops import native as N

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LENGTHS = (1, 255, 8192, 8193, 3 * 8192 + 5)      # one element, a partial chunk, one chunk exactly, +1, several + tail
GUARD = 8


def _wide(n, g):
    """Random sign, magnitude 10^U(-3, 3)."""
    mag = 10.0 ** (6.0 * torch.rand(n, generator=g) - 3.0)
    return mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def _slots(lengths, offs, align):
    """Start offsets of consecutive views in a flat buffer: view i starts ``offs[i]`` elements past a multiple of
    ``align`` elements, with at least GUARD untouched elements on both sides."""
    starts, cur = [], 0
    for n, o in zip(lengths, offs):
        cur = (cur + GUARD + align - 1) // align * align + o
        starts.append(cur)
        cur += n
    return starts, cur + GUARD


@pytest.mark.parametrize('scale', [1.0, 0.5, 1.0 / 3])
def test_multi_accumulate_bit_equals_cpu_replay(scale):
    """70 tensors in one call (past kCopyMaxT = 64: two launches), every length class, fp32 and bf16 sources, 16-byte
    aligned views and views at an odd element offset on either side (wide and element-wise paths); a zero-element
    pair in the middle; destinations without a source (None: they only take the scale); the guard elements around
    every destination view unchanged."""
    C = N.ensure_loaded()
    g = torch.Generator().manual_seed(17)
    lengths = [LENGTHS[i % 5] for i in range(70)]
    d_off = [(i // 5) % 2 for i in range(70)]                 # 0: aligned, 1: odd element offset
    s_off = [(i // 10) % 2 for i in range(70)]
    bf = [(i // 20) % 2 == 1 or i % 7 == 3 for i in range(70)]
    d_start, d_total = _slots(lengths, d_off, 4)
    s_start, s_total = _slots(lengths, s_off, 8)               # 8 elements: 16 bytes of bf16, 32 of fp32
    d_cpu = _wide(d_total, g)
    s32_cpu, s16_cpu = _wide(s_total, g), _wide(s_total, g).bfloat16()
    d_gpu, s32, s16 = d_cpu.to(DEV), s32_cpu.to(DEV), s16_cpu.to(DEV)
    assert d_gpu.data_ptr() % 16 == 0 and s32.data_ptr() % 16 == 0 and s16.data_ptr() % 16 == 0
    want = d_cpu.clone()
    sc = torch.tensor(scale, dtype=torch.float32)
    dsts, srcs = [], []
    for i, n in enumerate(lengths):
        if i == 33:
            dsts.append(torch.empty(0, device=DEV))
            srcs.append(torch.empty(0, device=DEV))
        src_cpu, src_gpu = (s16_cpu, s16) if bf[i] else (s32_cpu, s32)
        dsts.append(d_gpu[d_start[i]:d_start[i] + n])
        w = want[d_start[i]:d_start[i] + n]
        if i % 11 == 5:                                       # every length and both alignments among them
            srcs.append(None)
            w.copy_(w * sc)
            continue
        srcs.append(src_gpu[s_start[i]:s_start[i] + n])
        w.copy_((w + src_cpu[s_start[i]:s_start[i] + n].float()) * sc)
    assert len(dsts) == 71
    C.multi_accumulate(dsts, srcs, scale)
    torch.cuda.synchronize()
    got = d_gpu.cpu()
    assert torch.equal(got, want), int((got != want).sum())
    assert not torch.equal(got, d_cpu)


def test_multi_accumulate_checks_and_fallback():
    C = N.ensure_loaded()
    with pytest.raises(RuntimeError, match='fp32 destination'):
        C.multi_accumulate([torch.zeros(4, device=DEV, dtype=torch.bfloat16)], [torch.zeros(4, device=DEV)], 1.0)
    # a pair the copy would hand to copy_ (a non-dense destination): add_ + mul_, same arithmetic
    g = torch.Generator().manual_seed(3)
    d_cpu, s_cpu = _wide(64, g).view(8, 8), _wide(32, g).view(8, 4)
    d = d_cpu.to(DEV)
    C.multi_accumulate([d[:, :4]], [s_cpu.to(DEV)], 1.0 / 3)
    want = d_cpu.clone()
    want[:, :4] = (d_cpu[:, :4] + s_cpu) * torch.tensor(1.0 / 3, dtype=torch.float32)
    assert torch.equal(d.cpu(), want)


def test_reducer_keeps_g1_over_k_where_later_micro_batches_have_no_gradient():
    """A parameter with a gradient in micro-batch 1 only: nothing added, nothing zeroed, and the closing 1/k applied
    by the same native launch (a None source)."""
    from applestar_amd.parallel.dp import GradientReducer
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(300, 70, device=DEV))
    q = torch.nn.Parameter(torch.randn(9001, device=DEV))
    r = GradientReducer([p, q])
    x = torch.randn(70, device=DEV)
    l1 = (p @ x).sum() * 1.7 + (q * q).sum()
    l2, l3 = (p @ x).pow(2).sum(), (p @ x).sum() * 0.3
    gp = [torch.autograd.grad(l, p, retain_graph=True)[0] for l in (l1, l2, l3)]
    gq = torch.autograd.grad(l1, q, retain_graph=True)[0]
    r.backward(l1)
    r.backward(l2, accumulate=True, scale=1.0, no_collective=True)
    assert torch.equal(q.grad, gq)
    r.backward(l3, accumulate=True, scale=1.0 / 3)
    third = torch.tensor(1.0 / 3, dtype=torch.float32, device=DEV)
    assert torch.equal(p.grad, ((gp[0] + gp[1]) + gp[2]) * third)
    assert torch.equal(q.grad, gq * third)


@pytest.mark.parametrize('src_dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('scale', [1.0, 0.5, 1.0 / 3])
def test_multi_strided_accumulate_bit_equals_cpu_replay(scale, src_dtype):
    """Both forms of the strided kernel in one call: a channels_last [128, 64, 3, 3] gradient into its contiguous
    slot (the 4-D form) and a transposed [70, 130] one (the LDS tile form, past both tile edges: 64 rows, 128
    columns); guards around both destinations unchanged."""
    C = N.ensure_loaded()
    g = torch.Generator().manual_seed(23)
    shapes = [(128, 64, 3, 3), (70, 130)]
    n = [128 * 64 * 9, 70 * 130]
    starts, total = _slots(n, [0, 1], 4)
    d_cpu = _wide(total, g)
    src_cpu = [_wide(n[0], g).view(shapes[0]).to(src_dtype).contiguous(memory_format=torch.channels_last),
               _wide(n[1], g).view(130, 70).to(src_dtype).t()]
    assert src_cpu[1].shape == (70, 130) and src_cpu[1].stride() == (1, 70)
    d_gpu = d_cpu.to(DEV)
    src = [s.to(DEV) for s in src_cpu]
    assert [s.stride() for s in src] == [s.stride() for s in src_cpu]
    dsts = [d_gpu[a:a + k].view(sh) for a, k, sh in zip(starts, n, shapes)]
    want = d_cpu.clone()
    sc = torch.tensor(scale, dtype=torch.float32)
    for a, k, sh, s in zip(starts, n, shapes, src_cpu):
        w = want[a:a + k].view(sh)
        w.copy_((w + s.float()) * sc)
    spec = []
    for s in src:
        spec += N._view_spec(s, s)
    C.multi_strided_accumulate(dsts, src, spec, scale)
    torch.cuda.synchronize()
    got = d_gpu.cpu()
    assert torch.equal(got, want), int((got != want).sum())
    # and through accumulate_into, which sorts the pairs between the two launches itself
    from applestar_amd.parallel.dp import accumulate_into
    d2 = d_cpu.to(DEV)
    accumulate_into([d2[a:a + k].view(sh) for a, k, sh in zip(starts, n, shapes)], src, scale)
    assert torch.equal(d2.cpu(), want)


# ------------------------------------------------------------------ trainer windows
SEEDS = (11, 12, 13)


def _trainer(prec, lr=None):
    from applestar_amd.rl.trainer import RLTrainer
    torch.manual_seed(0)
    lc = {'use_value_feature': True, 'amp_dtype': 'bfloat16' if prec == 'bf16' else None}
    if lr is not None:
        lc['learning_rate'] = lr
    return RLTrainer({'learner': lc, 'model': {'enable_baselines': ['winloss']}}, device='cuda')


def _bufs(tr):
    """The gradient buffers the optimizer reads (not copies)."""
    if tr.master is not None:
        out = {'master': tr.master.master.grad}
        out.update({tr.master.names[p]: p.grad for p in tr.master.fp32_params})
        return out
    return {n: p.grad for n, p in tr.model.named_parameters() if p.requires_grad}


def _snap(tr):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in _bufs(tr).items()}


def _loss(tr, batch):
    from applestar_amd.runtime.train_engine import amp_context
    with amp_context(tr.device, tr.amp_dtype):
        out = tr.model.rl_learner_forward(**copy.deepcopy(batch))
    return tr.loss.compute_loss(out)['total_loss']


def _single(tr, batch):
    tr.backward(_loss(tr, batch))
    return _snap(tr)


def _replay(gs):
    k = len(gs)
    acc = gs[0].clone()
    for j, g in enumerate(gs[1:], start=2):
        acc = acc + g
        if j == k:
            acc = acc * torch.tensor(1.0 / k, dtype=torch.float32, device=acc.device)
    return acc


def _window(tr, batches):
    for b in batches[:-1]:
        tr.backward(_loss(tr, b), more=True)
    assert tr._window == len(batches) - 1
    tr.backward(_loss(tr, batches[-1]))
    assert tr._window == 0
    return _snap(tr)


@pytest.fixture(scope='module')
def batches():
    from applestar_amd.rl.synthetic import rl_batch, to_device
    N.ensure_loaded()
    return [to_device(rl_batch(2, 6, max_entities=96, seed=s), 'cuda') for s in SEEDS]


@pytest.fixture(scope='module')
def det_ctx(batches):
    """Deterministic mode: per (precision, phased) one trainer and the single-backward gradients of the three
    batches, computed once (the weights never change: no update runs on these trainers)."""
    prev = N.set_deterministic(True)
    cache = {}

    def get(prec, phased, monkeypatch):
        monkeypatch.setenv('APPLESTAR_PHASED_BACKWARD', phased)
        if (prec, phased) not in cache:
            tr = _trainer(prec)
            assert tr.model.phase_cut == (phased == '1')
            _single(tr, batches[0])                        # warm-up: derived weight forms, side streams
            g = [_single(tr, b) for b in batches]
            again = _single(tr, batches[0])
            assert all(torch.equal(g[0][k], again[k]) for k in again)      # the mode's promise; the replay needs it
            cache[(prec, phased)] = (tr, g)
        return cache[(prec, phased)]

    yield get
    cache.clear()
    N.set_deterministic(prev)


@pytest.mark.parametrize('k', [2, 3])
@pytest.mark.parametrize('phased', ['0', '1'])
def test_fp32_window_bit_equals_replay_deterministic(det_ctx, batches, phased, k, monkeypatch):
    tr, g = det_ctx('fp32', phased, monkeypatch)
    assert tr.master is None
    got = _window(tr, batches[:k])
    want = {n: _replay([gj[n] for gj in g[:k]]) for n in got}
    bad = [n for n in got if not torch.equal(got[n], want[n])]
    assert not bad, bad[:8]
    assert sum(float(v.abs().sum()) for v in got.values()) > 0.0


@pytest.mark.parametrize('phased,k', [('0', 2), ('1', 3)])
def test_bf16_window_accumulates_in_fp32_master_grad(det_ctx, batches, phased, k, monkeypatch):
    tr, g = det_ctx('bf16', phased, monkeypatch)
    assert tr.master is not None and tr.master.master.grad.dtype == torch.float32
    got = _window(tr, batches[:k])
    assert all(v.dtype == torch.float32 for v in got.values())
    want = {n: _replay([gj[n] for gj in g[:k]]) for n in got}
    bad = [n for n in got if not torch.equal(got[n], want[n])]
    assert not bad, bad[:8]
    assert float(got['master'].abs().sum()) > 0.0


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_window_and_update_bit_equal_the_mean_gradient_update(det_ctx, batches, prec, monkeypatch):
    """micro_step(A); step(B) on a fresh trainer, twice: identical weights, equal to a twin's whose buffers were set
    to the replayed mean gradient before _reduce(); _update(); the LSTM exchange healthy, every weight finite."""
    monkeypatch.setenv('APPLESTAR_PHASED_BACKWARD', '0')
    det_ctx(prec, '0', monkeypatch)                        # the mode is on while this fixture lives

    def weights(tr):
        torch.cuda.synchronize()
        return [tr.master.master.detach().clone()] + [p.detach().clone() for p in tr.master.fp32_params] \
            if tr.master is not None else [p.detach().clone() for p in tr.params]

    runs = []
    for _ in range(2):
        tr = _trainer(prec, lr=1e-3)
        w0 = weights(tr)
        i0 = tr.micro_step(dict(batches[0]))
        assert tr.iter == 0 and 'gradient' not in i0
        info = tr.step(dict(batches[1]))
        assert tr.iter == 1 and tr._window == 0
        assert float(info['lstm_exchange_ok']) == 1.0
        runs.append(weights(tr))
    assert all(bool(torch.isfinite(w).all()) for w in runs[0])
    assert any(not torch.equal(a, b) for a, b in zip(w0, runs[0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    twin = _trainer(prec, lr=1e-3)
    ga, gb = _single(twin, batches[0]), _single(twin, batches[1])
    with torch.no_grad():
        for n, buf in _bufs(twin).items():
            buf.copy_(_replay([ga[n], gb[n]]))
    twin._reduce()
    twin._update()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], weights(twin)))


def test_fp32_window_within_noise_floor_default_mode(batches, monkeypatch):
    """Default (atomic) kernels: the window's buffers against (gA + gB) * 0.5 by the rule of
    tests/test_phased_backward_gpu.py - max(tol * scale, 4 * noise, 1e-6 * top), the noise from A run twice."""
    monkeypatch.setenv('APPLESTAR_PHASED_BACKWARD', '0')
    prev = N.set_deterministic(False)
    try:
        tr = _trainer('fp32')
        _single(tr, batches[0])
        ga, ga2, gb = _single(tr, batches[0]), _single(tr, batches[0]), _single(tr, batches[1])
        got = _window(tr, batches[:2])
    finally:
        N.set_deterministic(prev)
    tol = 1e-5
    top = max(float(a.abs().max()) for a in ga.values())
    bad = {}
    for n, a in ga.items():
        want = (a + gb[n]) * 0.5
        scale = max(float(a.abs().max()), 1e-30)
        noise = float((a - ga2[n]).abs().max())
        err = float((got[n] - want).abs().max())
        if err > max(tol * scale, 4 * noise, 1e-6 * top):
            bad[n] = (err / scale, noise / scale, scale / top)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:8]
