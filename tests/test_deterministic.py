"""The deterministic-mode switch (``ops.set_deterministic``, ``APPLESTAR_DETERMINISTIC``, ``learner.deterministic``)
and the ordered CPU references the GPU kernels are compared against bit for bit.  Runs anywhere."""
import os
import subprocess
import sys

import pytest
import torch

from applestar_amd import ops
from applestar_amd.ops import native
from applestar_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def restore_flag():
    prev = native.deterministic()
    yield
    native.set_deterministic(prev)


def test_set_deterministic_round_trip(restore_flag):
    native.set_deterministic(False)
    assert ops.set_deterministic(True) is False          # returns the previous value
    assert ops.deterministic() is True and native.deterministic() is True
    assert ops.set_deterministic(0) is True
    assert ops.deterministic() is False


@pytest.mark.parametrize('value,want', [(None, 'False'), ('0', 'False'), ('1', 'True')])
def test_environment_default(value, want):
    env = {k: v for k, v in os.environ.items() if k != 'APPLESTAR_DETERMINISTIC'}
    if value is not None:
        env['APPLESTAR_DETERMINISTIC'] = value
    out = subprocess.run([sys.executable, '-c', 'from applestar_amd.ops import native; print(native.deterministic())'],
                         cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == want


def _cpu_trainer(deterministic):
    from applestar_amd.rl.trainer import RLTrainer
    torch.manual_seed(0)
    return RLTrainer({'learner': {'use_value_feature': True, 'deterministic': deterministic},
                      'model': {'enable_baselines': ['winloss']}}, device='cpu')


def test_learner_key_reaches_the_flag_and_cpu_step_is_unchanged(restore_flag):
    """``learner.deterministic: True`` turns the mode on when the engine is built and never turns it off; on CPU
    tensors the mode is a no-op: one trainer step gives identical weights with the flag on and off."""
    from applestar_amd.rl.synthetic import rl_batch
    from applestar_amd.rl.trainer import DEFAULT_LEARNER_CONFIG
    from applestar_amd.sl.trainer import DEFAULT_SL_CONFIG
    assert DEFAULT_LEARNER_CONFIG.learner.deterministic is False and DEFAULT_SL_CONFIG.learner.deterministic is False
    torch.set_num_threads(2)
    native.set_deterministic(False)
    off = _cpu_trainer(False)
    assert native.deterministic() is False
    info_off = off.step(rl_batch(1, 2, max_entities=16, seed=3))
    on = _cpu_trainer(True)
    assert native.deterministic() is True
    info_on = on.step(rl_batch(1, 2, max_entities=16, seed=3))
    _cpu_trainer(False)                                   # a later engine without the key leaves the mode on
    assert native.deterministic() is True
    assert float(info_on['total_loss']) == float(info_off['total_loss'])
    for (n, a), (_, b) in zip(on.model.named_parameters(), off.model.named_parameters()):
        assert torch.equal(a, b), n


def _wide(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (6.0 * torch.rand(*shape, generator=g) - 3.0)
    return mag * torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)


def test_scatter_connection_ordered_matches_index_add():
    """The ordered reference == the index_add_ reference to fp32 rounding (at most U - 1 roundings per element), with
    collisions, clamped coordinates and an all-masked observation; untouched pixels are +0."""
    B, U, C, H, W = 3, 70, 8, 8, 10
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, W + 40, (B, U), generator=g)
    y = torch.randint(0, H + 40, (B, U), generator=g)
    x[0], y[0] = torch.where(torch.arange(U) % 2 == 0, 3, 120), torch.where(torch.arange(U) % 2 == 0, 2, 100)
    proj = _wide(B, U, C, seed=8)
    proj[2] = 0
    got = R.scatter_connection_ordered(proj, x, y, H, W)
    ref = R.scatter_connection(proj.double(), x, y, H, W)
    mag = R.scatter_connection(proj.double().abs(), x, y, H, W)
    assert got.shape == (B, C, H, W) and got.dtype == torch.float32
    assert bool(((got.double() - ref).abs() <= 2.0 ** -24 * (U - 1) * mag).all())
    assert int((got[0].abs().sum(0) > 0).sum()) == 2 and float(got[2].abs().max()) == 0.0
    assert not bool(torch.signbit(got[mag == 0]).any())
    # the contractual order, spelled out for one colliding pixel
    acc = None
    for u in range(0, U, 2):
        acc = proj[0, u] if acc is None else acc + proj[0, u]
    assert torch.equal(got[0, :, 2, 3], acc)
    assert torch.equal(R.scatter_connection_ordered(proj.bfloat16(), x, y, H, W).float(),
                       R.scatter_connection_ordered(proj.bfloat16().float(), x, y, H, W).bfloat16().float())


def test_gather_steps_grad_ordered_matches_autograd():
    B, N1, S, C = 3, 10, 12, 32
    labels = torch.tensor([[4, 1, 4, 7, 4, 1, 0, 1, 2, 7, 7, 3], [N1 - 1] * S, [0, 0, 0, 5, 6, 5, 8, 5, 2, 2, 2, 9]])
    key = _wide(B, N1, C, seed=5).double().requires_grad_()
    dout = _wide(B, S, C, seed=6)
    ops.gather_steps(key, labels).backward(dout.double())           # CPU: torch.gather (scatter_add backward)
    got = R.gather_steps_grad_ordered(dout, labels, N1)
    mag = torch.zeros(B, N1, C, dtype=torch.float64).scatter_add_(1, labels.unsqueeze(-1).expand(B, S, C),
                                                                  dout.double().abs())
    assert bool(((got.double() - key.grad).abs() <= 2.0 ** -24 * (S - 1) * mag).all())
    assert float(got[1, :N1 - 1].abs().max()) == 0.0
    assert torch.equal(got[0, 4], (dout[0, 0] + dout[0, 2]) + dout[0, 4])
