"""Step-by-step oracle of the persistent selected-units sampler (csrc/kernels/pointer.hip) with every tensor the
binding ``su_sample`` returns, the comparator that judges a kernel's structure, picks and values, and the case table
of the binding-level GPU check (tests/test_su_sample_gpu.py; tests/test_su_sample_oracle.py proves the comparator).

One row at a time, from the binding's own arguments (the formulas are the header comment of pointer.hip):

    x_0 = relu(c0);  x_t = relu(c0 + bf + Wf he_{t-1})            qin_t = Wq2 x_t + bq2
    gates = LN_i(Wih qin_t) + LN_h(Whh h);  i, f, g, o = chunk(gates)
    c' = LN_c(sig(f) c + sig(i) tanh(g));  h' = sig(o) tanh(c')
    l_t[n] = (masked ? -1e9 : h' . key[n]) / T   n <= en;   masked: en at t = 0, the units picked before t
    r_t = searchsorted(cumsum(softmax(l_t)), u_t * total, right=True)
    emb = mean of the picked keys;  he_t = relu(We1 emb + be1);  the row stops when r_t = en

``form='wide'`` (su_sample_wide_kernel) reads he as a bf16 pair: hi, the fp32 value truncated to bf16, plus lo, the
round-to-nearest-even bf16 of the exact remainder.  In float64 that moves the logits by 2.6e-5, the size of the bound,
so the oracle of that form applies it; ``form='narrow'`` (su_sample_kernel) has no such step."""
import itertools
from collections import namedtuple

import torch

NEG = -1e9
MASKED = -1e8                   # a logit at or below this is a masked one (-1e9 in padding, -1e9 / T in live columns)
EXTRA_W = 513                   # width of the extra-units map
BAND = 1e-5                     # a pick is valid within this of a float64 CDF edge (test_kernels_gpu._same_or_boundary)
FLOOR = 8 * 2.0 ** -23          # of max|want|: a few fp32 ulps of the tensor's largest value (lnlstm_oracle.py)
# kernel error / fp32 host oracle error, the project's 4 (lnlstm_oracle.py, test_sl_loss_gpu.py).  Worst ratios
# measured on an MI355X over every case of CASES, against the plain fp32 oracle (torch.tanh / exp / log):
#   1,024 threads: logits 1.30, logp 1.00, emb 1.00        256 threads: logits 1.18, logp 1.13, emb 1.00
# so the wide kernel's fast_tanh (1 - 2 / (1 + e^2x)), __expf and __logf stay inside the host oracle's own rounding
# and the yardstick holds none of them.  For logp and emb the bound is FLOOR * max|want| in every case.
FACTOR = 4
WEIGHTS = ('wf', 'bf', 'wq2', 'bq2', 'wih', 'whh', 'lni_w', 'lni_b', 'lnh_w', 'lnh_b', 'lnc_w', 'lnc_b', 'we1', 'be1')
OUTPUTS = ('logits', 'results', 'logp', 'su_num', 'emb', 'extra')


def _ln(x, w, b, eps):
    xc = x - x.mean()
    return xc * (xc.pow(2).mean() + eps).rsqrt() * w + b


def split_he(he):
    """he as the wide kernel holds it: hi (the fp32 value with its low 16 bits cleared) + lo (RNE bf16 of he - hi)."""
    hi = (he.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(he.dtype)
    return hi, (he - hi).to(torch.bfloat16).to(he.dtype)


def row_bounds(inp, b):
    """(n1, en) of row b: entity_num clamped into the key tensor, as the kernel clamps it."""
    n1 = min(max(int(inp['entity_num'][b]), 0) + 1, inp['key'].shape[1])
    return n1, n1 - 1


def oracle(inp, dtype=torch.float64, form='narrow', picks=None, *, he_lo=True, mask_end0=True,
           mask_last=True, cnt_bias=0, move_pick=None, logp_max_cols=None, extra_ge=False, gate_order=(0, 1, 2, 3)):
    """The sampler on the CPU in ``dtype``.  ``inp``: the binding's arguments by name (``wf`` holds the values the
    kernel multiplies by, exact in bf16 for a kernel run; ``temperature`` enters as the fp32 value of 1 / T that the
    binding passes).  ``picks`` [B, S]: teacher-forced on them; None: the oracle samples for itself.  The
    keyword-only arguments differ from the sampler's only in the comparator's
    mutation checks.  Returns the binding's six outputs by name, with its shapes (float tensors in ``dtype``)."""
    assert form in ('wide', 'narrow')
    c = lambda k: inp[k].detach().to('cpu', dtype)
    key, c0, u = c('key'), c('c0'), c('u')
    wf, bf, wq2, bq2, wih, whh, lni_w, lni_b, lnh_w, lnh_b, lnc_w, lnc_b, we1, be1 = (c(k) for k in WEIGHTS)
    eps, S = inp['eps'], inp['max_steps']
    inv_t = float(torch.tensor(1.0 / inp['temperature'], dtype=torch.float32))
    B, N1, Q = key.shape
    assert u.shape == (B, S)
    logits = torch.full((B, S, N1), NEG, dtype=dtype)
    results = torch.zeros(B, S, dtype=torch.long)
    logp = torch.zeros(B, S, dtype=dtype)
    su_num = torch.zeros(B, dtype=torch.long)
    emb = torch.zeros(B, Q, dtype=dtype)
    extra = torch.zeros(B, EXTRA_W if inp['extra_units'] else 1, dtype=dtype)
    for b in range(B):
        if not int(inp['su_mask'][b]):
            continue
        n1, en = row_bounds(inp, b)
        k = key[b, :n1]
        sel = torch.zeros(n1, dtype=torch.bool)
        h = cs = torch.zeros(Q, dtype=dtype)
        ksum = torch.zeros(Q, dtype=dtype)
        he, cnt, last, ended = None, 0, None, False
        su_num[b] = S
        for t in range(S):
            x = torch.relu(c0[b] if t == 0 else c0[b] + bf + wf @ he)
            gates = _ln(wih @ (wq2 @ x + bq2), lni_w, lni_b, eps) + _ln(whh @ h, lnh_w, lnh_b, eps)
            chunks = gates.chunk(4)
            i, f, g, o = (chunks[j] for j in gate_order)
            cs = _ln(torch.sigmoid(f) * cs + torch.sigmoid(i) * torch.tanh(g), lnc_w, lnc_b, eps)
            h = torch.sigmoid(o) * torch.tanh(cs)
            masked = sel.clone()
            if not mask_last and last is not None:
                masked[last] = False
            if t == 0 and mask_end0:
                masked[en] = True
            l = torch.where(masked, torch.full_like(k[:, 0], NEG), k @ h) * inv_t
            logits[b, t, :n1] = l
            if picks is None:
                cdf = torch.cumsum(torch.softmax(l, 0), 0)
                r = min(int(torch.searchsorted(cdf, u[b, t] * cdf[-1], right=True)), n1 - 1)
                if move_pick is not None:
                    r = move_pick(r, en, masked)
            else:
                r = int(picks[b, t])
            results[b, t] = last = r
            if logp_max_cols is None:
                logp[b, t] = torch.log_softmax(l, 0)[r]
            else:       # the maximum of the leading columns only, against the sum taken in the row's scale
                logp[b, t] = l[r] - l[:logp_max_cols].max() - torch.log(torch.exp(l - l.max()).sum())
            sel[r] = True
            if r == en:
                su_num[b] = t + 1
                ended = True
                break
            cnt += 1
            ksum = ksum + k[r]
            emb[b] = ksum / (cnt + cnt_bias)
            he = torch.relu(we1 @ emb[b] + be1)
            if form == 'wide':
                hi, lo = split_he(he)
                he = hi + lo if he_lo else hi
        if inp['extra_units'] and not ended:
            last_l = logits[b, S - 1, :n1]
            extra[b, :n1] = (last_l >= last_l[en] if extra_ge else last_l > last_l[en]).to(dtype)
    return dict(logits=logits, results=results, logp=logp, su_num=su_num, emb=emb, extra=extra)


# ---------------------------------------------------------------------------------------------- the comparator
class Mismatch(AssertionError):
    """args: (part, what, findings) with part one of 'structure', 'picks', 'values'."""

    @property
    def part(self):
        return self.args[0]


def _structure(got, inp):
    """Exact properties of the kernel's own results and logits; returns the findings."""
    bad = []
    lg, res, lp, su, emb, extra = (got[k] for k in OUTPUTS)
    B, N1, _ = inp['key'].shape
    S = inp['max_steps']
    want_shapes = dict(logits=(B, S, N1), results=(B, S), logp=(B, S), su_num=(B,), emb=(B, 32),
                       extra=(B, EXTRA_W if inp['extra_units'] else 1))
    for k, s in want_shapes.items():
        if tuple(got[k].shape) != s:
            bad.append((k, 'shape', tuple(got[k].shape), s))
    if bad:
        return bad
    cols = torch.arange(N1)
    for b in range(B):
        n1, en = row_bounds(inp, b)
        s = int(su[b])
        want_extra = torch.zeros(extra.shape[1])
        if not int(inp['su_mask'][b]):
            if s != 0:
                bad.append((b, 'su_num of a row without selection', s))
            if emb[b].abs().max() != 0:
                bad.append((b, 'emb of a row without selection'))
            s = 0
        else:
            ends = torch.nonzero(res[b] == en).flatten()
            want_s = int(ends[0]) + 1 if len(ends) else S
            if s != want_s:
                bad.append((b, 'su_num', s, want_s))
                s = max(0, min(s, S))
            r = res[b, :s].tolist()
            if any(not 0 <= v < n1 for v in r):
                bad.append((b, 'pick out of range', r))
                continue
            if len(set(r)) != len(r):
                bad.append((b, 'unit picked twice', r))
            if r and r[0] == en:
                bad.append((b, 'end token picked at step 0'))
            for t in range(s):
                want_masked = cols >= n1
                want_masked[res[b, :t]] = True
                if t == 0:
                    want_masked[en] = True
                if not torch.equal(lg[b, t] <= MASKED, want_masked):
                    diff = torch.nonzero((lg[b, t] <= MASKED) != want_masked).flatten().tolist()
                    bad.append((b, t, 'masked columns differ at', diff[:8]))
            if inp['extra_units'] and not len(ends):
                want_extra[:n1] = (lg[b, S - 1, :n1] > lg[b, S - 1, en]).float()
        if not bool((lg[b, s:] <= MASKED).all()):
            bad.append((b, 'logits of steps not run'))
        if bool(res[b, s:].any()) or bool(lp[b, s:].any()):
            bad.append((b, 'results / logp of steps not run'))
        if not torch.equal(extra[b].float(), want_extra):
            bad.append((b, 'extra differs at', torch.nonzero(extra[b].float() != want_extra).flatten().tolist()[:8]))
    return bad


def cdf_edges(row, r):
    """float64 softmax CDF of a logits row just below and at column r."""
    cdf = torch.cumsum(torch.softmax(row.double(), 0), 0)
    return (float(cdf[r - 1]) if r > 0 else 0.0), float(cdf[r])


def _picks(got, inp):
    """Every pick is an unmasked column whose float64 CDF interval, widened by BAND, holds the row's uniform."""
    bad = []
    for b in range(inp['key'].shape[0]):
        n1, _ = row_bounds(inp, b)
        for t in range(int(got['su_num'][b])):
            row, r, u = got['logits'][b, t, :n1], int(got['results'][b, t]), float(inp['u'][b, t])
            if not float(row[r]) > MASKED:
                bad.append((b, t, r, 'masked column picked'))
                continue
            lo, hi = cdf_edges(row, r)
            if not lo - BAND <= u <= hi + BAND:
                bad.append((b, t, r, f'u {u:.9f} outside [{lo:.9f}, {hi:.9f}]'))
    return bad


_TEACHER = {}


def teacher(inp, form, picks):
    """(float64, fp32) oracles of ``form`` teacher-forced on ``picks``: computed once per process for the same
    inputs (by identity: ``inputs`` hands out one dict per case), form and picks, and left unchanged."""
    k = (id(inp), form, picks.numpy().tobytes())
    if k not in _TEACHER:
        _TEACHER[k] = (inp, oracle(inp, torch.float64, form, picks), oracle(inp, torch.float32, form, picks))
    return _TEACHER[k][1:]


def check(got, inp, form, what=''):
    """The kernel's six outputs ``got`` (by name) for the inputs ``inp``.  Structure: exact, from the kernel's own
    results and logits.  Picks: each within BAND of its interval of the float64 CDF of the kernel's own logits row.
    Values: logits (unmasked entries of the steps run) and emb against the float64 oracle teacher-forced on the
    kernel's picks, logp against the float64 log-softmax of the kernel's own logits row;
    max|got - want| <= max(FACTOR * max|host - want|, FLOOR * max|want|) with host the same in fp32.
    Raises Mismatch naming the first part that fails; returns {tensor: (kernel err, host err, bound)}."""
    got = {k: got[k].detach().cpu() for k in OUTPUTS}
    for part, fn in (('structure', _structure), ('picks', _picks)):
        bad = fn(got, inp)
        if bad:
            raise Mismatch(part, what, bad[:12])
    want, host = teacher(inp, form, got['results'])
    assert torch.equal(want['su_num'], got['su_num']) and torch.equal(host['su_num'], got['su_num'])
    B, S = got['results'].shape
    run = torch.arange(S)[None, :] < got['su_num'][:, None]                  # [B, S]
    live = run[:, :, None] & (want['logits'] > MASKED)
    lsm = {}
    for dt in (torch.float64, torch.float32):
        ls = torch.log_softmax(got['logits'].to(dt), -1).gather(2, got['results'][:, :, None]).squeeze(2)
        lsm[dt] = torch.where(run, ls, torch.zeros_like(ls))
    triples = {'logits': (got['logits'][live], want['logits'][live], host['logits'][live]),
               'emb': (got['emb'], want['emb'], host['emb']),
               'logp': (got['logp'], lsm[torch.float64], lsm[torch.float32])}
    rows, bad = {}, []
    for k, (g, w, h) in triples.items():
        ek = float((g.double() - w).abs().max()) if w.numel() else 0.0
        eh = float((h.double() - w).abs().max()) if w.numel() else 0.0
        bound = max(FACTOR * eh, FLOOR * float(w.abs().max()) if w.numel() else 0.0)
        ratio = ek / eh if eh > 0 else float('inf') if ek > 0 else 0.0
        print(f'{what} {k} kernel err {ek:.3e} host err {eh:.3e} bound {bound:.3e} ratio {ratio:.2f}')
        rows[k] = (ek, eh, bound)
        if not ek <= bound:           # a NaN misses too
            bad.append((k, ek, eh, bound))
    if bad:
        raise Mismatch('values', what, bad)
    return rows


# ---------------------------------------------------------------------------------------------- the case table
Case = namedtuple('Case', 'key_dtype temperature max_steps extra_units')
# both key dtypes x both temperatures x the three step counts with the extra-units map, and the 7-step case (where
# almost every row never ends) without it
CASES = [Case(d, t, s, True) for d, t, s in itertools.product(('fp32', 'bf16'), (1.0, 0.8), (64, 7, 1))] + \
        [Case(d, 1.0, 7, False) for d in ('fp32', 'bf16')]
case_id = lambda c: f'{c.key_dtype}-T{c.temperature}-S{c.max_steps}-{"extra" if c.extra_units else "noextra"}'

STRIDE = 513                     # key rows per batch row: the LDS key planes at their full pitch
# one below, at and one above every 64-entity wave of the wide form and 192-entity wave of the 256-thread form: the
# end token of these rows sits in lane 0, 1 or 63 of its wave, where its scan prefix is the wave's offset or total
ENTITY_NUMS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 383, 384, 385, 511, 512)
FORCED_END = (64, 192, 384, 512)  # a second row each that draws its end token at step 5, alone in its wave
END_STEP = 5
# the end token inside a 16-lane row of its wave (and inside a 3-entity chunk of the 256-thread form), with masked
# lanes of the same wave behind it: there the masked token's prefix is summed in another order than the total
MID_ROW = (10, 40, 62, 100, 104, 164, 300)
ROW_NO_SELECTION = len(ENTITY_NUMS) + len(FORCED_END) + len(MID_ROW)      # su_mask = 0
ROW_CLAMPED = ROW_NO_SELECTION + 1                          # entity_num = 600, beyond the stride: clamped to 512
U_LAST = 1 - 2.0 ** -24          # the largest fp32 uniform
SEED = 5                         # every condition of test_su_sample_oracle.py holds at it; at others (3, 6, 7, 8) a
                                 # row ends before it has drawn from each of its 64-entity blocks


def make_inputs(case, seed=SEED):
    """CPU fp32 inputs of a case, by the binding's argument names.  The LN_h gain is 0.25 * (1 + 0.1 randn) for the
    reason in lnlstm_oracle.make_inputs: at gain 1 a random recurrence amplifies rounding over 64 steps and the
    yardstick becomes noise.  Every row draws with u = 1 - 2^-24 at step 0 (unit en - 1 in float64: the last wave
    that holds mass, with an all-masked wave behind it when n1 = 65, 129, 193, 385, 513) and u = 0 at step 1
    (unit 0).  The random draws do not depend on the case, so a 7-step case is the start of the 64-step one."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    en = list(ENTITY_NUMS) + list(FORCED_END) + list(MID_ROW) + [100, 600]
    B = len(en)
    d = dict(key=rn(B, STRIDE, 32), c0=rn(B, 256), u=torch.rand(B, 64, generator=g),
             wf=(rn(256, 256) / 16).bfloat16().float(), bf=0.1 * rn(256), wq2=rn(32, 256) / 16, bq2=0.1 * rn(32),
             wih=rn(128, 32) / 32 ** 0.5, whh=rn(128, 32) / 32 ** 0.5,
             lni_w=1 + 0.1 * rn(128), lni_b=0.1 * rn(128), lnh_w=0.25 * (1 + 0.1 * rn(128)), lnh_b=0.1 * rn(128),
             lnc_w=1 + 0.1 * rn(32), lnc_b=0.1 * rn(32), we1=rn(256, 32) / 32 ** 0.5, be1=0.1 * rn(256))
    d['u'][:, 0] = U_LAST
    d['u'][:, 1] = 0
    d['u'][len(ENTITY_NUMS):len(ENTITY_NUMS) + len(FORCED_END), END_STEP] = U_LAST
    d['u'] = d['u'][:, :case.max_steps].contiguous()
    if case.key_dtype == 'bf16':
        d['key'] = d['key'].bfloat16().float()       # rounded once: the same values reach both sides
    d['entity_num'] = torch.tensor(en)
    d['su_mask'] = torch.ones(B, dtype=torch.uint8)
    d['su_mask'][ROW_NO_SELECTION] = 0
    d.update(temperature=case.temperature, eps=1e-5, max_steps=case.max_steps, extra_units=case.extra_units)
    return d


_INPUTS = {}


def inputs(case):
    """The inputs of a case, made once per process and left unchanged."""
    if case not in _INPUTS:
        _INPUTS[case] = make_inputs(case)
    return _INPUTS[case]


def run_kernel(C, inp, key_dtype, dev='cuda'):
    """The binding on fresh contiguous device copies of ``inp`` with the keys in ``key_dtype`` ('fp32' / 'bf16');
    returns the six outputs by name on the CPU."""
    d = lambda k, dt: inp[k].to(dev, dt).contiguous()
    out = C.su_sample(d('key', {'fp32': torch.float32, 'bf16': torch.bfloat16}[key_dtype]), d('c0', torch.float32),
                      d('u', torch.float32),
                      d('entity_num', torch.long), d('su_mask', torch.uint8), d('wf', torch.bfloat16),
                      *(d(k, torch.float32) for k in WEIGHTS[1:]), float(inp['temperature']), float(inp['eps']),
                      int(inp['max_steps']), bool(inp['extra_units']))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in zip(OUTPUTS, out)}
