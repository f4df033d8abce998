"""DAPO end to end on the CPU: the successive KL in the reference head statistics and the torch loss, the
learner data path (synthetic batch, model output, collate), the league's successive checkpoints and the
actor's successive model (local and through the inference server)."""
import os
import random

import pytest
import torch

from refutil import reference_available, import_reference
from applestar_amd.ops import reference as R
from applestar_amd.rl.loss import ReinforcementLoss, HEADS
from applestar_amd.rl.synthetic import rl_batch
from applestar_amd.models.model import Model

DAPO_W = {'action_type': 1.0, 'delay': 0.5, 'queued': 2.0, 'selected_units': 0.25, 'target_unit': 1.5,
          'target_location': 0.75}


def _leaves(x, path=()):
    if torch.is_tensor(x):
        yield path, x
    elif isinstance(x, dict):
        for k, v in x.items():
            yield from _leaves(v, path + (k,))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _leaves(v, path + (i,))


# ---------------------------------------------------------------------------- reference head_stats
def test_reference_head_stats_successive_matches_float64():
    g = torch.Generator().manual_seed(0)
    Rr, C = 9, 31
    l = 3 * torch.randn(Rr, C, generator=g)
    t = 3 * torch.randn(Rr, C, generator=g)
    u = 3 * torch.randn(Rr, C, generator=g)
    for x in (l, t, u):
        x[:, 20:] = -1e9
        x[4] = -1e9                                   # fully masked row: uniform, KL 0
    a = torch.randint(0, 20, (Rr,), generator=g)
    three = R.head_stats(l, t, a)
    four = R.head_stats(l, t, a, u)
    assert len(three) == 3 and len(four) == 4
    for x, y in zip(three, four[:3]):
        assert torch.equal(x, y)
    lp = torch.log_softmax(l.double(), -1)
    ulp = torch.log_softmax(u.double(), -1)
    want = (ulp.exp() * (ulp - lp)).sum(-1)
    assert four[3].dtype == torch.float32
    assert (four[3].double() - want).abs().max().item() < 1e-5
    assert float(four[3][4]) == 0.0
    no_teacher = R.head_stats(l, None, a, u)
    assert torch.equal(no_teacher[2], torch.zeros(Rr)) and torch.equal(no_teacher[3], four[3])


# ---------------------------------------------------------------------------- torch-path loss
@pytest.fixture(scope='module')
def model_out():
    torch.manual_seed(0)
    cfg = {'learner': {'use_value_feature': True}, 'model': {'enable_baselines': ['winloss']}}
    model = Model(cfg, use_value_network=True)
    batch = rl_batch(2, 3, max_entities=30, seed=1, successive=True)
    with torch.no_grad():
        out = model.rl_learner_forward(**batch)
    plain = dict(rl_batch(2, 3, max_entities=30, seed=1))
    with torch.no_grad():
        out_plain = model.rl_learner_forward(**plain)
    return out, out_plain


def _dapo_cfg(steps):
    return {'use_dapo': True, 'loss_weights': {'dapo': 0.1}, 'dapo_head_weights': DAPO_W,
            'dapo': {'dapo_steps': steps}}


def _gate(out):
    step = out['step']
    steps = float(step.flatten().sort().values[step.numel() // 2])      # the median: both flag values occur
    flag = (step < steps)
    assert flag.any() and not flag.all()
    return steps, flag


def test_torch_loss_dapo_matches_float64_formula(model_out):
    out, _ = model_out
    steps, flag = _gate(out)
    info = ReinforcementLoss(_dapo_cfg(steps)).compute_loss(dict(out, value=dict(out['value'])))
    su_mask = out['mask']['selected_units_mask'].double()
    total = 0.0
    for h in HEADS:
        lp = torch.log_softmax(out['target_logit'][h].double(), -1)
        ulp = torch.log_softmax(out['successive_logit'][h].double(), -1)
        kl = (ulp.exp() * (ulp - lp)).sum(-1)
        if h == 'selected_units':
            kl = (kl * su_mask).sum(-1)
        if h not in ('action_type', 'delay'):
            kl = kl * out['mask']['actions_mask'][h].double()
        want = float((kl * flag.double()).mean())
        assert abs(float(info['dapo/' + h]) - want) <= 1e-4 * max(1.0, abs(want)), h
        total += want * DAPO_W[h]
    assert abs(float(info['dapo/total']) - total) <= 1e-4 * max(1.0, abs(total))
    off = ReinforcementLoss(dict(_dapo_cfg(steps), use_dapo=False)).compute_loss(dict(out, value=dict(out['value'])))
    assert 'dapo/total' not in off
    assert abs(float(info['total_loss']) - float(off['total_loss']) - 0.1 * total) <= 1e-4 * max(1.0, abs(total))


@pytest.mark.skipif(not reference_available(), reason='reference tree not available')
def test_torch_loss_dapo_matches_reference_dapo_loss(model_out):
    import_reference()
    import distar.agent.default.rl_training.as_rl_utils as ref
    out, _ = model_out
    steps, _ = _gate(out)
    info = ReinforcementLoss(_dapo_cfg(steps)).compute_loss(dict(out, value=dict(out['value'])))
    lps = {h: torch.log_softmax(out['target_logit'][h].float(), -1) for h in HEADS}
    total, d = ref.dapo_loss(lps, out['successive_logit'], out['mask'], out['step'], steps, DAPO_W)
    for h in HEADS:
        r = d['battle/' + h]
        assert abs(float(info['dapo/' + h]) - r) <= 1e-4 * max(1.0, abs(r)), h
    assert abs(float(info['dapo/total']) - float(total)) <= 1e-4 * max(1.0, abs(float(total)))


def test_dapo_player_gating(model_out):
    out, out_plain = model_out
    steps, _ = _gate(out)
    x = lambda o: dict(o, value=dict(o['value']))  # noqa: E731
    base = ReinforcementLoss(_dapo_cfg(steps)).compute_loss(x(out_plain))
    assert not any(k.startswith('dapo/') for k in base)
    exploiter = ReinforcementLoss(_dapo_cfg(steps), player_id='EP0').compute_loss(x(out))
    none = ReinforcementLoss(_dapo_cfg(steps)).compute_loss(x(dict(out, successive_logit=None)))
    for other in (exploiter, none):
        assert set(other) == set(base)
        assert torch.equal(other['total_loss'], base['total_loss'])


# ---------------------------------------------------------------------------- learner data path
def test_rl_batch_stable_without_successive():
    a = dict(_leaves(rl_batch(2, 3, max_entities=30, seed=5)))
    b = dict(_leaves(rl_batch(2, 3, max_entities=30, seed=5, successive=False)))
    c = dict(_leaves(rl_batch(2, 3, max_entities=30, seed=5, successive=True)))
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], c[k]), k
    extra = set(c) - set(a)
    assert extra == {('successive_logit', h) for h in HEADS}
    for h in HEADS:
        t, u = c[('teacher_logit', h)], c[('successive_logit', h)]
        assert t.shape == u.shape and torch.equal(t <= -1e8, u <= -1e8) and not torch.equal(t, u)


def test_model_output_carries_successive_only_when_given(model_out):
    out, out_plain = model_out
    assert 'successive_logit' in out and 'successive_logit' not in out_plain
    assert set(out) - set(out_plain) == {'successive_logit'}


def _fake_traj(T, n_ent, seed):
    """Trajectory steps with just the keys _pad_step reads (entities, action / teacher leaves)."""
    g = torch.Generator().manual_seed(seed)
    steps = []
    for t in range(T + 1):
        n = n_ent + t
        st = {'entity_info': {'unit_type': torch.randint(0, 5, (n,), generator=g)}, 'entity_num': torch.tensor(n),
              'hidden_state': [(torch.zeros(4), torch.zeros(4))]}
        if t < T:
            s = 1 + t % 3
            tl = {'action_type': torch.randn(7, generator=g), 'selected_units': torch.randn(s, n + 1, generator=g),
                  'target_unit': torch.randn(n, generator=g)}
            st.update({'selected_units_num': torch.tensor(s),
                       'action_info': {'selected_units': torch.randint(0, n, (s,), generator=g)},
                       'behaviour_logp': {'selected_units': -torch.rand(s, generator=g)},
                       'teacher_logit': tl, 'successive_logit': {k: v.clone() for k, v in tl.items()},
                       'mask': {}})
        steps.append(st)
    return steps


def test_collate_pads_successive_like_teacher():
    from applestar_amd.agent.collate import collate_trajectories
    trajs = [_fake_traj(3, 4, 0), _fake_traj(3, 9, 1)]
    b = collate_trajectories(trajs)
    N = b['entity_info']['unit_type'].shape[1]
    assert b['successive_logit']['selected_units'].shape == (3, 2, 64, N + 1)
    assert b['successive_logit']['target_unit'].shape == (3, 2, N)
    for k in b['teacher_logit']:
        assert torch.equal(b['teacher_logit'][k], b['successive_logit'][k]), k
    assert (b['successive_logit']['selected_units'][0, 0, 1:] == -1e9).all()
    for tr in trajs:                                  # steps without the key: the batch has none either
        for st in tr:
            st.pop('successive_logit', None)
    assert 'successive_logit' not in collate_trajectories(trajs)


# ---------------------------------------------------------------------------- league
def _league_cfg(ckpts, use_dapo, players=('MP0', 'EP0')):
    n = len(players)
    return {'learner': {'use_dapo': use_dapo},
            'league': {'active_players': {'checkpoint_path': [ckpts[p] for p in players], 'player_id': list(players),
                                          'pipeline': ['default'] * n, 'frac_id': [1] * n, 'z_prob': [0.0] * n,
                                          'teacher_id': ['t'] * n, 'teacher_path': ['none'] * n,
                                          'z_path': ['3map.json'] * n, 'one_phase_step': [1000] * n,
                                          'chosen_weight': [1] * n},
                       'historical_players': {'player_id': ['sl'], 'checkpoint_path': ['none'], 'pipeline': ['default'],
                                              'frac_id': [1], 'z_prob': [0.0], 'z_path': ['3map.json']},
                       'stat_warm_up_size': 5, 'payoff_min_win_rate_games': 2, 'save_resume_freq': 1e9,
                       'scalar_log': False}}


def _marker(path):
    return int(torch.load(path, weights_only=True)['marker'])


def test_league_successive_checkpoints_rotate(tmp_path):
    from applestar_amd.league.league import League
    random.seed(0)
    ckpts = {}
    for p in ('MP0', 'EP0'):
        ckpts[p] = str(tmp_path / f'{p}_init.pth.tar')
        torch.save({'marker': torch.tensor(0)}, ckpts[p])
    lg = League(_league_cfg(ckpts, True), root=str(tmp_path), start_threads=False)
    mp0 = lg.active_players['MP0']
    d = os.path.join(lg.model_dir, 'successive_model', 'MP0')
    assert os.path.isdir(d)
    served = mp0.successive_model_path
    assert os.path.dirname(served) == d and _marker(served) == 0      # first save: the copy just made is served
    # two updates past one_phase_step / 2: the copy made at save k is served at save k + 1
    for k, marker in ((1, 0), (2, 1)):
        torch.save({'marker': torch.tensor(k)}, mp0.checkpoint_path)
        before = mp0.last_successive_step
        lg.learner_send_train_info({'player_id': 'MP0', 'train_steps': 501, 'checkpoint_path': ''})
        assert mp0.last_successive_step == before + 501 == mp0.total_agent_step
        assert mp0.successive_model_path == served and _marker(served) == marker
    # an update short of half a phase saves nothing
    torch.save({'marker': torch.tensor(3)}, mp0.checkpoint_path)
    lg.learner_send_train_info({'player_id': 'MP0', 'train_steps': 10, 'checkpoint_path': ''})
    assert _marker(served) == 1
    seen = set()
    for _ in range(40):
        job = lg.actor_ask_for_job({'job_type': 'train'})
        assert len(job['successive_checkpoint_paths']) == len(job['player_ids']) == len(job['successive_ids'])
        for pid, path in zip(job['player_ids'], job['successive_checkpoint_paths']):
            if pid == 'MP0' and 'eval' not in job['branch']:
                assert path == served
                seen.add(pid)
            else:
                assert path == 'none', (pid, job['branch'])
                seen.add(pid)
    assert {'MP0', 'EP0'} <= seen
    # resume: path and step persist, and the load is one more save (the copy of save 2 becomes the served file)
    cfg = _league_cfg(ckpts, True)
    cfg['league']['resume_path'] = lg.save_resume()
    lg.close()
    lg2 = League(cfg, root=str(tmp_path), start_threads=False)
    mp2 = lg2.active_players['MP0']
    assert mp2.successive_model_path == served and mp2.last_successive_step == mp2.total_agent_step == 1012
    assert _marker(served) == 2
    lg2.close()


def test_league_writes_nothing_without_dapo(tmp_path):
    from applestar_amd.league.league import League
    random.seed(0)
    ckpts = {}
    for p in ('MP0', 'EP0'):
        ckpts[p] = str(tmp_path / f'{p}_init.pth.tar')
        torch.save({'marker': torch.tensor(0)}, ckpts[p])
    lg = League(_league_cfg(ckpts, False), root=str(tmp_path), start_threads=False)
    lg.learner_send_train_info({'player_id': 'MP0', 'train_steps': 501, 'checkpoint_path': ''})
    assert not os.path.exists(os.path.join(lg.model_dir, 'successive_model'))
    assert lg.active_players['MP0'].last_successive_step == 0
    for _ in range(10):
        job = lg.actor_ask_for_job({'job_type': 'train'})
        assert set(job['successive_checkpoint_paths']) == {'none'}
    lg.close()


# ---------------------------------------------------------------------------- actor
class _StopAfter:
    """Control pipe stand-in for run_episodes: says 'close' once ``box`` holds a trajectory."""

    def __init__(self, box):
        self.box = box

    def poll(self):
        return bool(self.box)

    def recv(self):
        return 'close'


def _actor_cfg(use_dapo=True):
    from applestar_amd.actor.actor import DEFAULT_ACTOR_CONFIG
    from applestar_amd.utils.config import deep_merge_dicts
    return deep_merge_dicts(DEFAULT_ACTOR_CONFIG, {
        'actor': {'job_type': 'train_test', 'traj_len': 2, 'fake_model': False, 'player_ids': ['MP0'],
                  'successive_player_ids': ['MP0'], 'successive_model_paths': {}},
        'agent': {'z_path': '3map.json'},
        'env': {'player_ids': ['agent1', 'bot7'], 'game_steps_per_episode': 400, 'fake': True, 'random_seed': 0},
        'learner': {'use_dapo': use_dapo}})


@pytest.fixture(scope='module')
def successive_ckpt(tmp_path_factory):
    torch.manual_seed(3)
    path = str(tmp_path_factory.mktemp('succ') / 'MP0_successive.pth.tar')
    torch.save({'model': Model().state_dict(), 'last_iter': 7}, path)
    return path


def _check_traj(traj):
    assert len(traj) == 3
    for st in traj[:-1]:
        assert set(st['successive_logit']) == set(st['teacher_logit'])
        for h, t in st['teacher_logit'].items():
            assert st['successive_logit'][h].shape == t.shape, h
        # another model than the teacher (here the policy itself): other logits
        assert not torch.equal(st['successive_logit']['action_type'], st['teacher_logit']['action_type'])
    assert 'successive_logit' not in traj[-1]


def test_actor_local_successive_model(successive_ckpt):
    from applestar_amd.actor.actor import run_episodes, _job_from_config
    torch.manual_seed(0)
    random.seed(0)
    cfg = _actor_cfg()
    cfg.actor.successive_model_paths = {'MP0': successive_ckpt}
    job = _job_from_config(cfg)
    assert job['successive_ids'] == ['MP0', 'none'] and job['successive_checkpoint_paths'] == [successive_ckpt, 'none']
    box = []
    run_episodes(cfg, job, send_traj=lambda traj, pid: box.append(traj), ctrl=_StopAfter(box))
    _check_traj(box[0])
    # the trajectory ring's batch assembly carries the successive leaves like the host collate
    from applestar_amd.agent.collate import collate_trajectories
    from applestar_amd.runtime.traj_ring import TrajectoryRing
    from applestar_amd.utils import serialize
    ref = collate_trajectories([box[0]])
    ring = TrajectoryRing(64 << 20, device='cpu')
    got = ring.batch([ring.put(serialize.dumps(box[0]))])
    assert set(got['successive_logit']) == set(ref['successive_logit'])
    for h, x in ref['successive_logit'].items():
        assert torch.equal(got['successive_logit'][h].to(x.dtype), x), h
    # DAPO off: the same job loads no successive model
    box2 = []
    run_episodes(_actor_cfg(False), job, send_traj=lambda traj, pid: box2.append(traj), ctrl=_StopAfter(box2))
    assert all('successive_logit' not in st for st in box2[0])


class _LoopbackClient:
    """InferenceClient stand-in that asks an in-process CPU server (same reply as over a routed pipe)."""

    def __init__(self, srv, route):
        self.srv, self.route = srv, route
        self.player_id, self.kind, self.teacher_id = route[:3]
        self.successive_id = route[3] if len(route) > 3 else None

    def infer(self, model_input):
        from applestar_amd.utils import serialize
        L = self.srv._launch(self.route, frames=[serialize.dumps(model_input)])
        frames = self.srv._reply_frames(L)
        if frames is None:
            return self.srv._results(L)[0]
        return serialize.loads(frames[0])


def test_actor_successive_through_inference_server(successive_ckpt):
    from applestar_amd.actor.actor import run_episodes, _job_from_config, load_policy_weights
    from applestar_amd.actor.inference import InferenceServer
    torch.manual_seed(0)
    random.seed(0)
    cfg = _actor_cfg()
    cfg.actor.successive_model_paths = {'MP0': successive_ckpt}
    job = _job_from_config(cfg)
    srv = InferenceServer('cpu')
    pol, succ = Model(cfg).eval(), Model(cfg).eval()
    assert load_policy_weights(succ, successive_ckpt) == 7
    srv.set_model('MP0', pol)
    srv.set_model('MP0', pol, teacher=True)
    srv.set_model('MP0', succ, successive=True)
    assert srv.successive['MP0'] is succ and srv.teachers['MP0'] is pol
    route = ('MP0', 'policy+teacher', 'MP0', 'MP0')
    box = []
    run_episodes(cfg, job, clients={('MP0', 'policy'): _LoopbackClient(srv, route)},
                 send_traj=lambda traj, pid: box.append(traj), ctrl=_StopAfter(box))
    _check_traj(box[0])
    assert route in srv._runners


def test_three_tuple_route_still_serves():
    from applestar_amd.actor.inference import InferenceServer
    from test_inference_server import _requests, _close
    torch.manual_seed(0)
    pol, tea, succ = Model().eval(), Model().eval(), Model().eval()
    srv = InferenceServer('cpu')
    srv.set_model('p', pol)
    srv.set_model('t', tea, teacher=True)
    srv.set_model('s', succ, successive=True)
    reqs = _requests(2, 1)
    hs = lambda: [(torch.randn(384) * 0.1, torch.randn(384) * 0.1) for _ in range(3)]  # noqa: E731
    reqs = [dict(r, teacher_hidden_state=hs()) for r in reqs]
    three = srv._results(srv._launch(('p', 'policy+teacher', 't'), inputs=reqs, keep_logits=True))
    assert all('teacher' in o and 'successive' not in o for o in three)
    four = srv._forward('p', 'policy+teacher', [dict(r, successive_hidden_state=hs()) for r in reqs],
                        teacher_id='t', successive_id='s')
    for a, b, r in zip(three, four, reqs):
        b = dict(b)
        su = b.pop('successive')
        _close(a, b)
        n, s = int(b['entity_num']), int(b['selected_units_num'])
        assert su['logit']['target_unit'].shape == (n,) and su['logit']['selected_units'].shape == (s, n + 1)
        assert su['logit']['action_type'].shape == b['teacher']['logit']['action_type'].shape
        assert not torch.equal(su['logit']['action_type'], b['teacher']['logit']['action_type'])
        assert len(su['hidden_state']) == 3
